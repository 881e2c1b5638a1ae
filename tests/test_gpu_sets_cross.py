"""An unbiased loss per parameter set from the one trace (drt_hip_render_param_sets_cross): k_path_sets_cross -- the parameter-set form's
operations on the path plus every set's sums of squares --, reduced by k_sets_cross_finish.  Per set the loss is a U-statistic over each
pixel's samples -- the mean over ordered pairs of DIFFERENT samples of (L_s - t)(L_s' - t) --, and out_bias is what was subtracted from
drt_hip_render_param_sets' plain loss.

Exact parity with the ordered-pair sums of the host's own samples is tests/test_sets_cross_host_api.py.  Here: the bits the call shares with
the parameter-set form, agreement with the cross-sample normal equations on the context's own parameters, padding, determinism, shards,
device pointers, sample ranges, f32 against f64, refusals, the statistics over 1000 seeds at 2 spp, and the loop built on it.

Bounds (tests/test_gpu_cross.py's): 1e-12 of the sum of absolute terms between two reductions of the same per-pixel values, 1e-9 (F64_TOL)
between f64 results formed differently, 1e-4 (GRAD_TOL) f32 against f64, 2e-4 (PIXEL_TOL) per pixel.  The sum of absolute terms of a
correction is not observable per pixel (S2 does not leave the device); it is bounded from BELOW by what the images give, v + 2 m^2 / (n - 1)
per pixel for var / n (v the variance image: S2 = v n (n - 1) + n m^2), so every bound here is at least as tight as the one on the true
terms."""
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
W, H = 23, 11                    # three full pixel groups and one of 61 lanes
KEYS = ("loss", "bias", "images", "variance")


def target_for(cam, seed=6):
    return np.random.RandomState(seed).uniform(0, 0.6, (cam.height, cam.width, 3)).astype(np.float32)


def three_sets(scene, seed):
    """tests/test_gpu_param_sets.py's: random in (0.05, 0.95), set 1 with a parameter at exactly 0 in one channel, set 2 with its last
    parameter (the emission of the Cornell rooms) above 1"""
    P = np.random.RandomState(seed).uniform(0.05, 0.95, (3, scene.n_params, 3))
    P[1, 0, 1] = 0.0
    P[2, scene.n_params - 1] = (1.7, 0.9, 1.3)
    return P


def sets_cross(hip, cam, rp, P, target, f64=False):
    return hip.render_param_sets_cross(cam, rp, P, target, f64=f64, images=True, variance=True)


def scales(res, target, n):
    """the sums of absolute terms of loss and bias per set and channel ([K,3] each; lower bounds: the module's docstring)"""
    m = res["images"].astype(np.float64)
    r = m - target.astype(np.float64)
    var = (np.abs(res["variance"].astype(np.float64)) + 2 * m * m / (n - 1)).sum((1, 2))
    return {"loss": (r * r).sum((1, 2)) + var, "bias": var}


def close(got, want, scale, tol, what):
    err = np.abs(np.asarray(got) - np.asarray(want))
    worst = float((err / np.maximum(scale, 1e-300)).max())
    print(f"{what}: {worst:.3e} of the sum of absolute terms")
    assert (err <= tol * scale + 1e-300).all(), (what, worst)


@pytest.mark.parametrize("f64", (False, True))
@pytest.mark.parametrize("name", SCENES)
def test_bits_shared_with_the_parameter_set_form(pkg, hip, name, f64):
    """the path kernel is the parameter-set form plus the sums of squares: in the library's kernels the images are render_param_sets' bit for
    bit and loss + bias is its loss to 1e-12 of the sum of absolute terms; bias > 0; the variance image is nonnegative up to rounding and
    sums to bias; one path launch, the forward render's segments.  A kernel hiprtc makes (caller-defined kinds) is another compile of the
    same source than the parameter-set form's: F64_TOL in f64, the project's f32 bounds in f32"""
    scene = pkg.scene_by_name(name)
    cam = camera_for(pkg, name, W, H)
    rp = pkg.RenderParams(spp=5, seed=9, **TRACER)
    hip.upload_scene(scene)
    P = three_sets(scene, 11)
    target = target_for(cam)
    got = sets_cross(hip, cam, rp, P, target, f64)
    plain = hip.render_param_sets(cam, rp, P, target=target, f64=f64)
    fwd = hip.render(cam, rp)[2]
    assert got["stats"]["kernels"]["path"]["launches"] == 1
    assert got["stats"]["segments"] == plain["stats"]["segments"] == fwd["segments"] > 0
    library = got["stats"]["path_program"] != "specialised"
    assert library == ("coslobe" not in name)
    sc = scales(got, target, rp.spp)
    if library:
        assert np.array_equal(got["images"], plain["images"])
    else:
        assert np.abs(got["images"] - plain["images"]).max() <= (F64_TOL if f64 else PIXEL_TOL) * np.abs(plain["images"]).max()
    close(got["loss"] + got["bias"], plain["loss"], sc["loss"], 1e-12 if library else (F64_TOL if f64 else GRAD_TOL), "loss + bias")
    assert (got["bias"] > 0).all()
    v = got["variance"].astype(np.float64)
    assert v.min() >= -1e-6 * v.max() and v.max() > 0
    assert np.abs(v.sum((1, 2)) - got["bias"]).max() <= 1e-6 * got["bias"].max()


@pytest.mark.parametrize("f64", (False, True))
@pytest.mark.parametrize("name", SCENES)
def test_against_the_cross_sample_normal_equations(pkg, hip, name, f64):
    """with set 0 the context's own parameters, loss[0], bias[0] and variance[0] are render_normal_equations_cross' loss, bias[:, K] and
    variance on the same camera, render parameters and target: another path kernel (it forms L through its zero-channel masks) and another
    reduction -- 1e-9 of the sum of absolute terms in f64, GRAD_TOL in f32, the variance image per pixel at F64_TOL / PIXEL_TOL of its
    largest value"""
    scene = pkg.scene_by_name(name)
    cam = camera_for(pkg, name, W, H)
    rp = pkg.RenderParams(spp=5, seed=9, **TRACER)
    hip.upload_scene(scene)
    own = np.asarray(scene.params, dtype=np.float64)
    P = np.concatenate([own[None], three_sets(scene, 11)[:2]])
    target = target_for(cam)
    got = sets_cross(hip, cam, rp, P, target, f64)
    ne = hip.render_normal_equations_cross(cam, rp, directions(scene, 1, 11), target, f64=f64, images=True, variance=True)
    assert got["stats"]["segments"] == ne["stats"]["segments"] > 0
    sc = scales(got, target, rp.spp)
    tol = F64_TOL if f64 else GRAD_TOL
    close(got["loss"][0], ne["loss"], sc["loss"][0], tol, "loss[0]")
    close(got["bias"][0], ne["bias"][:, 1], sc["bias"][0], tol, "bias[0]")
    vmax = np.abs(ne["variance"]).max()
    assert vmax > 0 and np.abs(got["variance"][0] - ne["variance"]).max() <= (F64_TOL if f64 else PIXEL_TOL) * vmax
    assert np.abs(got["images"][0] - ne["image"]).max() <= (F64_TOL if f64 else PIXEL_TOL) * np.abs(ne["image"]).max()


def test_padding_and_companions(pkg, hip):
    """a set's loss, bias, image and variance depend neither on its companions, nor on its position, nor on n_sets, bit for bit: n_sets = 1,
    3 and the cap run the kernels of width 2, 4 and 8"""
    scene = pkg.scene_by_name("params20")
    cam = pkg.cornell_camera(W, H)
    hip.upload_scene(scene)
    target = target_for(cam)
    rs = np.random.RandomState(3)
    p0 = rs.uniform(0.05, 0.95, (scene.n_params, 3))
    others = rs.uniform(0.05, 0.95, (pkg.MAX_SETS_CROSS - 1, scene.n_params, 3))
    assert pkg.MAX_SETS_CROSS == 8
    for f64 in (False, True):
        rp = pkg.RenderParams(spp=5, seed=2, **TRACER)
        one = sets_cross(hip, cam, rp, p0[None], target, f64)
        a = sets_cross(hip, cam, rp, np.stack([p0, others[0], others[1]]), target, f64)
        b = sets_cross(hip, cam, rp, np.stack([others[2], p0, others[3]]), target, f64)
        cap = sets_cross(hip, cam, rp, np.concatenate([others, p0[None]]), target, f64)
        assert np.abs(one["images"]).max() > 0 and (one["bias"] > 0).all()
        for res, k in ((a, 0), (b, 1), (cap, pkg.MAX_SETS_CROSS - 1)):
            for key in KEYS:
                assert np.array_equal(res[key][k], one[key][0]), (key, k, f64)
        # (and the companions are not copies of it)
        assert not np.array_equal(a["loss"][1], a["loss"][0]) and not np.array_equal(cap["images"][0], cap["images"][7])


def test_determinism_shards_device_pointers(pkg, hip):
    """identical calls give identical bits; three shards (bands of 4 rows) tile the images and variance exactly and their sums add up to the
    whole frame's within 1e-12; device pointers give the host-buffer bits, with and without the optional outputs"""
    scene = pkg.scene_by_name("cornell_specular")
    cam = pkg.cornell_camera(W, H)
    hip.upload_scene(scene)
    P = three_sets(scene, 19)
    target = target_for(cam)
    rp = pkg.RenderParams(spp=5, seed=2, **TRACER)
    for f64 in (False, True):
        n1 = sets_cross(hip, cam, rp, P, target, f64)
        n2 = sets_cross(hip, cam, rp, P, target, f64)
        for key in KEYS:
            assert np.array_equal(n1[key], n2[key]), key
        tiles = {k: np.zeros_like(n1[k]) for k in KEYS}
        for shard in range(3):
            ns = sets_cross(hip, cam, dataclasses.replace(rp, shard=shard, n_shards=3, band_rows=4), P, target, f64)
            for k in KEYS:
                tiles[k] += ns[k]
        for k in ("images", "variance"):
            assert np.array_equal(tiles[k], n1[k]), k
        sc = scales(n1, target, rp.spp)
        for k in ("loss", "bias"):
            close(tiles[k], n1[k], sc[k], 1e-12, f"three shards, {k}")
    K = 3
    f = DeviceFrames([(H, W, 3), (K, H, W, 3), (K, H, W, 3)])
    d = DeviceFrames([(K, 3), (K, 3)], np.float64)
    try:
        f.put(0, target)
        hip.render_param_sets_cross_device(cam, rp, P, f.ptrs[0].value, d.ptrs[0].value, out_bias_ptr=d.ptrs[1].value,
                                           out_images_ptr=f.ptrs[1].value, out_variance_ptr=f.ptrs[2].value)
        hip.synchronize()
        want = sets_cross(hip, cam, rp, P, target)
        assert np.array_equal(f.get(1), want["images"]) and np.array_equal(f.get(2), want["variance"])
        assert np.array_equal(d.get(0), want["loss"]) and np.array_equal(d.get(1), want["bias"])
        d.put(0, np.zeros((K, 3)))
        hip.render_param_sets_cross_device(cam, rp, P, f.ptrs[0].value, d.ptrs[0].value)
        hip.synchronize()
        assert np.array_equal(d.get(0), want["loss"])
    finally:
        hip.synchronize()
        f.free()
        d.free()


def test_sample_ranges():
    """raw moments add across sample ranges: spp 7 from a process where DRT_HIP_PATH_SPR=3 cuts it into ranges of 3, 3 and 1 samples against
    a process with the default plan (tests/sets_cross_child.py), f32 and f64: loss and bias within 1e-12 of the sum of absolute terms, the
    images and the variance image -- fp64 sums added in another order, then rounded to the float the ABI carries -- within one unit in
    the last place of a float at their largest value (2^-23 of it)"""
    child = os.path.join(ROOT, "tests", "sets_cross_child.py")

    def run(spr):
        env = dict(os.environ)
        env.pop("DRT_HIP_PATH_SPR", None)
        if spr:
            env["DRT_HIP_PATH_SPR"] = str(spr)
        r = subprocess.run([sys.executable, child], capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return json.loads(r.stdout.strip().split("\n")[-1])

    default, three = run(0), run(3)
    for mode in ("f32", "f64"):
        a, b = default[mode], three[mode]
        print(mode, "ranges", a["ranges"], b["ranges"])
        assert b["ranges"] == 3 and a["ranges"] != 3
        for k in ("loss", "bias"):
            close(np.array(b[k]), np.array(a[k]), np.array(a["scale_" + k]), 1e-12, f"{mode}: ranges of 3, 3, 1 samples, {k}")
        for k in ("images", "variance"):
            x, y = np.array(a[k]), np.array(b[k])
            assert np.abs(x - y).max() <= 2.0 ** -23 * np.abs(x).max(), (mode, k)


def test_f32_against_f64(pkg, hip):
    """loss and bias of the f32 render within GRAD_TOL of the f64 render's, relative to the sum of absolute terms, on a frame whose f32 and
    f64 segment counts are equal (no path took another surface): the first such seed of 9 ... 13"""
    for name in ("cornell", "cornell_specular"):
        scene = pkg.scene_by_name(name)
        cam = camera_for(pkg, name, W, H)
        hip.upload_scene(scene)
        P = three_sets(scene, 11)
        target = target_for(cam)
        for seed in range(9, 14):
            rp = pkg.RenderParams(spp=5, seed=seed, **TRACER)
            n64 = sets_cross(hip, cam, rp, P, target, True)
            n32 = sets_cross(hip, cam, rp, P, target, False)
            if n64["stats"]["segments"] == n32["stats"]["segments"]:
                break
            print(f"{name}, seed {seed}: {n32['stats']['segments']} segments in f32, {n64['stats']['segments']} in f64")
        else:
            pytest.fail(f"{name}: no seed of 9 ... 13 with equal segment counts")
        sc = scales(n64, target, rp.spp)
        for k in ("loss", "bias"):
            close(n32[k], n64[k], sc[k], GRAD_TOL, f"{name}, seed {seed}, {k}")


def test_refusals_leave_the_context_usable(pkg, hip):
    """every refusal with its status and the words "param sets cross"; after each of them a plain render returns the bits it returned before"""
    scene = pkg.cornell_box()
    cam = pkg.cornell_camera(W, H)
    rp = pkg.RenderParams(spp=3, seed=4, min_bounces=3, absorb=1.0)
    hip.upload_scene(scene)
    P = np.random.RandomState(37).uniform(0.05, 0.95, (3, scene.n_params, 3))
    target = target_for(cam)
    before = hip.render(cam, rp, backward=True)[:2]
    cross_before = sets_cross(hip, cam, rp, P, target)

    def same_as_before():
        img, g, _ = hip.render(cam, rp, backward=True)
        assert np.array_equal(img, before[0]) and np.array_equal(g, before[1])

    cd = cam.to_desc()
    cap = pkg.MAX_SETS_CROSS
    imgs = np.zeros((cap, cam.height, cam.width, 3), np.float32)
    var = np.zeros((cap, cam.height, cam.width, 3), np.float32)
    loss, bias = np.zeros((cap, 3)), np.zeros((cap, 3))
    ip, vp, lp, bp, tp = (a.ctypes.data_as(C.c_void_p) for a in (imgs, var, loss, bias, target))
    INVALID, UNSUPPORTED = -1, -6                    # DRT_ERR_INVALID, DRT_ERR_UNSUPPORTED (include/drt_hip.h)
    words = "param sets cross"

    def refused(status, more, n, sets, rp_=rp, target_p=tp, loss_p=lp, flags=0):
        """straight through the C ABI (the Python mirror refuses shapes, counts and values before the call); then the context is what it was"""
        d = rp_.to_desc()
        d.flags = rp_.flags | flags
        sp = np.ascontiguousarray(sets, dtype=np.float64).ctypes.data_as(C.c_void_p) if sets is not None else None
        rc = hip.lib.drt_hip_render_param_sets_cross(hip.ctx, C.byref(cd), C.byref(d), n, sp, target_p, ip, loss_p, bp, vp, None)
        msg = hip.lib.drt_hip_last_error(hip.ctx).decode()
        assert rc == status and words in msg and all(w in msg for w in more), (rc, msg)
        same_as_before()

    for spp in (1, 0):
        refused(INVALID, ["spp"], 3, P, rp_=dataclasses.replace(rp, spp=spp))
    with pytest.raises(ValueError, match=f"{words}.*spp"):
        sets_cross(hip, cam, dataclasses.replace(rp, spp=1), P, target)
    refused(INVALID, ["NULL", "target"], 3, P, target_p=None)
    with pytest.raises(ValueError, match=f"{words}.*target"):
        sets_cross(hip, cam, rp, P, None)
    refused(INVALID, ["NULL", "out_loss"], 3, P, loss_p=None)
    refused(INVALID, ["NULL", "param_sets"], 3, None)
    for n, sets in ((0, P), (cap + 1, np.full((cap + 1, scene.n_params, 3), 0.5))):
        refused(INVALID, ["n_sets"], n, sets)
    with pytest.raises(ValueError, match=f"{words}.*n_sets"):
        sets_cross(hip, cam, rp, np.full((cap + 1, scene.n_params, 3), 0.5), target)
    Pbad = P.copy()
    Pbad[1, 2, 1] = np.nan
    refused(INVALID, ["finite"], 3, Pbad)
    tb = target.copy()
    tb[3, 4, 1] = np.nan
    refused(INVALID, ["finite"], 3, P, target_p=tb.ctypes.data_as(C.c_void_p))
    refused(INVALID, ["BACKWARD"], 3, P, flags=pkg.RENDER_BACKWARD)
    h = hip.render_async(cam, rp)
    with pytest.raises(pkg.DrtHipError, match=f"DRT_ERR_INVALID.*{words}.*in flight"):
        sets_cross(hip, cam, rp, P, target)
    hip.wait(h)
    same_as_before()
    for flag in (pkg.RENDER_UNFUSED, pkg.RENDER_UNBIASED, pkg.RENDER_LOSS_L2, pkg.RENDER_ALLREDUCE, pkg.RENDER_ALLREDUCE_ASYNC):
        refused(UNSUPPORTED, [], 3, P, flags=flag)
    refused(UNSUPPORTED, ["bounces_per_launch"], 3, P, rp_=dataclasses.replace(rp, bounces_per_launch=1))
    # the call works, gives what it gave, and leaves the context's parameters alone
    again = sets_cross(hip, cam, rp, P, target)
    assert all(np.array_equal(again[k], cross_before[k]) for k in KEYS)
    same_as_before()
    # a mesh, more parameters than the kernels stage, a group context
    mesh = pkg.scene_by_name("mesh6x8")
    hip.upload_scene(mesh)
    with pytest.raises(pkg.DrtHipError, match=f"DRT_ERR_UNSUPPORTED.*{words}.*mesh"):
        sets_cross(hip, cam, rp, np.full((2, mesh.n_params, 3), 0.5), target)
    hip.render(cam, rp, backward=True)
    hip.upload_scene(scene)
    same_as_before()
    big = pkg.cornell_box()
    for k in range(140):
        big.parameter((0.5, 0.5, 0.5), True, f"spare{k}")
    hip.upload_scene(big)
    with pytest.raises(pkg.DrtHipError, match=f"DRT_ERR_UNSUPPORTED.*{words}.*136"):
        sets_cross(hip, cam, rp, np.full((2, big.n_params, 3), 0.5), target)
    hip.render(cam, rp)
    hip.upload_scene(scene)
    same_as_before()
    group = pkg.HipRenderer([0, 0])
    try:
        group.upload_scene(scene)
        with pytest.raises(pkg.DrtHipError, match=f"DRT_ERR_UNSUPPORTED.*{words}.*group"):
            sets_cross(group, cam, rp, P, target)
        group.render(cam, rp, backward=True)
    finally:
        group.close()
    same_as_before()


def test_unbiased_per_set_where_the_plain_losses_are_not(pkg, hip):
    """The statistics, on tests/test_gpu_cross.py::test_unbiased_where_the_plain_values_are_not's recipe.  cornell, 16 x 14, depth 5,
    n = 2 spp, f32; the target is a render at 8192 spp under 0.7 x the red and green albedos; the sets are 1.0 x, 0.85 x and 0.7 x those
    albedos.  G = 1000 calls with seeds 100 ... 1099.  The truth uses no code of this form and is free of bias: per set, 8 PAIRS of
    render_param_sets images at 4096 spp on different seeds (9000 ...), sum_x (m_a - t)(m_b - t) per pair, their mean and standard error.
      - every mean(loss~) is within 5 sqrt(se^2 + se_truth^2) of the truth;
      - every mean(loss~ + bias) is at least 8 of its own standard errors off it.
    Printed too: the plain and the unbiased differences between sets 0 and 2 under common paths, with their standard errors.
    (On the CPU, from the restatement, the same recipe with a pixel's two samples taken from 1-spp renders of seeds 500000 apart: the
    unbiased losses -0.06 ... -0.33 combined standard errors off the truth, the plain ones 92 ... 110 of their own; set 0 - set 2, red
    channel: truth 0.00347, unbiased 0.00270 +- 0.00120, plain 0.1246 +- 0.0020.)"""
    scene = pkg.cornell_box()
    cam = pkg.cornell_camera(16, 14)
    names = list(scene.param_names)
    own = np.asarray(scene.params, dtype=np.float64)
    P = np.stack([own] * 3)
    for k, f in enumerate((1.0, 0.85, 0.7)):
        for p in (names.index("red"), names.index("green")):
            P[k, p] = f * own[p]
    dimmed = pkg.cornell_box()
    dimmed.params = [tuple(float(x) for x in v) for v in P[2]]
    hip.upload_scene(dimmed)
    target = hip.render(cam, pkg.RenderParams(spp=8192, seed=77, **TRACER))[0].copy()
    hip.upload_scene(scene)
    t64 = target.astype(np.float64)
    pairs = []
    for i in range(8):
        a = hip.render_param_sets(cam, pkg.RenderParams(spp=4096, seed=9000 + 2 * i, **TRACER), P, double=True)["images"]
        b = hip.render_param_sets(cam, pkg.RenderParams(spp=4096, seed=9001 + 2 * i, **TRACER), P, double=True)["images"]
        pairs.append(((a - t64) * (b - t64)).sum((1, 2)))
    pairs = np.stack(pairs)                                  # [8, K, 3]
    truth, se_t = pairs.mean(0), pairs.std(0, ddof=1) / np.sqrt(8.0)
    G = 1000
    un, pl = [], []
    for seed in range(100, 100 + G):
        res = hip.render_param_sets_cross(cam, pkg.RenderParams(spp=2, seed=seed, **TRACER), P, target)
        un.append(res["loss"])
        pl.append(res["loss"] + res["bias"])
    un, pl = np.stack(un), np.stack(pl)                      # [G, K, 3]
    se_u, se_p = un.std(0, ddof=1) / np.sqrt(G), pl.std(0, ddof=1) / np.sqrt(G)
    z_u = (un.mean(0) - truth) / np.sqrt(se_u * se_u + se_t * se_t)
    z_p = (pl.mean(0) - truth) / se_p
    print("truth [set, channel]:\n", truth, "\n its standard error:\n", se_t)
    print("unbiased loss, combined standard errors off the truth:\n", z_u, "\nplain loss (loss + bias), its standard errors off the truth:\n", z_p)
    du, dp = un[:, 0] - un[:, 2], pl[:, 0] - pl[:, 2]
    print("set 0 - set 2 under common paths, truth", truth[0] - truth[2], "\n unbiased", du.mean(0), "+-", du.std(0, ddof=1) / np.sqrt(G),
          "\n plain   ", dp.mean(0), "+-", dp.std(0, ddof=1) / np.sqrt(G))
    assert (np.abs(z_u) <= 5).all()
    assert (np.abs(z_p) >= 8).all()


def test_the_loop_prices_its_candidates_on_one_trace(pkg):
    """tools/fit_albedo.py --gauss-newton --one-render --cross --lambda-sets 3 at 32 x 32 x 8, three steps: two traces per step by the tool's
    own counters (one normal_equations_cross, one param_sets_cross of the current point and three candidates); every accepted step's
    candidate had the lower loss~ on its trace, and a rejected step kept its point; the run is deterministic.  (No bound on where red lands.)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import fit_albedo
    start = np.array([0.2, 0.2, 0.2])
    runs = []
    for _ in range(2):
        dev = fit_albedo.DeviceRender(pkg, 32, 8, 8)
        try:
            rgb, hist, trace = fit_albedo.fit_gauss_newton_cross_sets(dev, 0, start, 3, 3)
            assert dev.calls == 6 and dev.traces_of_sets == 3
        finally:
            dev.close()
        assert len(hist) == len(trace) == 3
        prev = start
        for h, t in zip(hist, trace):
            assert t["losses"].shape == (4,) and 1 <= t["best"] <= 3 and t["losses"][t["best"]] == t["losses"][1:].min()
            assert t["accepted"] == bool(t["losses"][t["best"]] < t["losses"][0])
            if not t["accepted"]:
                assert np.array_equal(h, prev)
            prev = h
        runs.append((rgb, hist, [t["losses"] for t in trace]))
    print("fitted red", runs[0][0], "accepted", [t["accepted"] for t in trace])
    assert np.array_equal(runs[0][0], runs[1][0])
    for a, b in zip(runs[0][1] + runs[0][2], runs[1][1] + runs[1][2]):
        assert np.array_equal(a, b)
