"""k_path_lean (csrc/drt_path.h): the lockstep f32 column-form k_path with two more facts compiled in -- the render has no roulette inside the
loop (absorb == 1 at min_bounces == the depth cap), and no shape of the scene both scatters and emits.  The host takes it whenever both hold
(shard_plan: PathForm::fixed, ::no_lit_bxdf) and k_path as before whenever one does not.

1. Bit for bit against k_path, in one process.  Tracer A (absorb = 1, min_bounces = 6) takes the new kernel.  Tracer B (absorb = 0.5,
   min_bounces = 6, max_depth = 6) has a user cap, so it takes k_path; no vertex inside its loop sees the roulette either and its draw
   indices are A's, so it traces the same paths with the same arithmetic: image and gradients byte-identical, segments equal (capped_paths
   differ: B counts the paths its cap cut short).  On the parent commit, where both run k_path, A and B are byte-identical.
2. Renders and scenes without one of the facts run what they ran: a wall that also emits, a roulette inside the loop -- against the queue
   route (bounces_per_launch = 1) within the bounds tests/test_gpu_path_roles.py uses for the two routes, one k_path launch each.
3. Sample ranges of several samples (DRT_HIP_PATH_SPR is read once per process: a child, tests/path_lean_child.py): 6 spp in two ranges of
   3, A against B bit for bit there, and against this process's one-sample ranges within the two routes' bounds."""
import dataclasses
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import path_lean_child as plc
from test_gpu_path_roles import room

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def render_ab(pkg, scene, mode, backward):
    cam = pkg.cornell_camera(plc.W, plc.H)
    out = {}
    r = pkg.HipRenderer(0)
    try:
        r.set_specialisation(mode)
        r.upload_scene(scene)
        for name, rp in plc.tracers(pkg).items():
            out[name] = r.render(cam, rp, backward=backward)
    finally:
        r.close()
    return out


def assert_same_bits(a, b, backward, what):
    assert a[2]["kernels"]["path"]["launches"] == 1 and b[2]["kernels"]["path"]["launches"] == 1, what
    assert a[2]["path_program"] == b[2]["path_program"], what
    assert a[2]["segments"] == b[2]["segments"], (what, a[2]["segments"], b[2]["segments"])
    assert a[0].tobytes() == b[0].tobytes(), (what, float(np.abs(a[0] - b[0]).max()))
    if backward:
        assert a[1].tobytes() == b[1].tobytes(), (what, float(np.abs(a[1] - b[1]).max()))
        assert np.abs(a[1]).min() > 0, what
    assert a[2]["capped_paths"] == 0 and b[2]["capped_paths"] > 0, (what, a[2]["capped_paths"], b[2]["capped_paths"])


# the reference's scene through the library's kernels -- its own kinds compiled in (never / now: "builtin") and the kind-sorted program
# (generic) --, and a ten-shape room through the kernel hiprtc makes for it (its own kinds and roles compiled in, both entry points)
@pytest.mark.parametrize("backward", [False, True], ids=["fwd", "bwd"])
@pytest.mark.parametrize("scene_name,mode,program", [("cornell", "never", "builtin"), ("cornell", "now", "builtin"), ("cornell", "generic", "sorted"),
                                                     ("room", "never", "sorted"), ("room", "now", "specialised")])
def test_no_roulette_in_the_loop_compiled_in_keeps_every_bit(pkg, scene_name, mode, program, backward):
    scene = pkg.cornell_box() if scene_name == "cornell" else room(pkg, "plain")
    m = {"never": pkg.SPECIALISE_NEVER, "now": pkg.SPECIALISE_NOW, "generic": pkg.SPECIALISE_GENERIC}[mode]
    out = render_ab(pkg, scene, m, backward)
    assert out["A"][2]["path_program"] == program
    print(scene_name, mode, "bwd" if backward else "fwd", "segments", out["A"][2]["segments"], "capped", out["B"][2]["capped_paths"])
    assert_same_bits(out["A"], out["B"], backward, (scene_name, mode, backward))


def check_against_queue_route(pkg, scene, rp, mode):
    cam = pkg.cornell_camera(plc.W, plc.H)
    r = pkg.HipRenderer(0)
    try:
        r.set_specialisation(mode)
        r.upload_scene(scene)
        ref = r.render(cam, dataclasses.replace(rp, bounces_per_launch=1), backward=True)
        got = r.render(cam, rp, backward=True)
        fwd_ref = r.render(cam, dataclasses.replace(rp, bounces_per_launch=1))
        fwd = r.render(cam, rp)
    finally:
        r.close()
    assert ref[2]["kernels"]["path"]["launches"] == 0 and got[2]["kernels"]["path"]["launches"] == 1
    assert fwd_ref[2]["kernels"]["path"]["launches"] == 0 and fwd[2]["kernels"]["path"]["launches"] == 1
    print("segments", got[2]["segments"], ref[2]["segments"], "grad err / max", np.abs(got[1] - ref[1]).max() / np.abs(ref[1]).max())
    assert abs(got[2]["segments"] - ref[2]["segments"]) <= 64 and abs(fwd[2]["segments"] - fwd_ref[2]["segments"]) <= 64
    np.testing.assert_allclose(got[0], ref[0], rtol=2e-5, atol=1e-7)
    np.testing.assert_allclose(fwd[0], fwd_ref[0], rtol=2e-5, atol=1e-7)
    np.testing.assert_allclose(got[1], ref[1], rtol=2e-5, atol=1e-6 * np.abs(ref[1]).max())
    return got


@pytest.mark.parametrize("mode", ["never", "now"])
def test_a_wall_that_also_emits_keeps_k_path(pkg, mode):
    """the ten-shape room with the back wall given the light's emitter as well: its emission is added at every bounce that meets it"""
    scene = room(pkg, "plain")
    kind, material, emitter, p = scene.shapes[4]
    assert material >= 0 and emitter < 0
    scene.shapes[4] = (kind, material, scene.shapes[8][2], p)
    plain = room(pkg, "plain")
    rp = pkg.RenderParams(spp=plc.SPP, min_bounces=plc.DEPTH, absorb=1.0, seed=plc.SEED)
    got = check_against_queue_route(pkg, scene, rp, pkg.SPECIALISE_NOW if mode == "now" else pkg.SPECIALISE_NEVER)
    assert got[2]["path_program"] == ("specialised" if mode == "now" else "sorted")
    # (the wall's emission is in the image: the room without it is darker)
    r = pkg.HipRenderer(0)
    try:
        r.upload_scene(plain)
        dark = r.render(pkg.cornell_camera(plc.W, plc.H), rp)
    finally:
        r.close()
    assert got[0].mean() > 1.5 * dark[0].mean()


def test_a_roulette_inside_the_loop_keeps_k_path(pkg):
    rp = pkg.RenderParams(spp=plc.SPP, min_bounces=1, absorb=0.5, seed=plc.SEED)
    check_against_queue_route(pkg, pkg.cornell_box(), rp, pkg.SPECIALISE_NEVER)


def test_sample_ranges_of_several_samples(pkg):
    env = {k: v for k, v in os.environ.items() if not k.startswith("DRT_HIP_")}
    env["DRT_HIP_PATH_SPR"] = "3"
    d = tempfile.mkdtemp(prefix="drt_path_lean_")
    try:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "path_lean_child.py"), d], capture_output=True, text=True, env=env, timeout=240)
        assert p.returncode == 0, f"child: status {p.returncode}\n" + p.stdout[-3000:] + p.stderr[-3000:]
        with np.load(os.path.join(d, "outputs.npz")) as z:
            child = {k: z[k] for k in z.files}
    finally:
        shutil.rmtree(d, ignore_errors=True)
    r = pkg.HipRenderer(0)
    try:
        r.upload_scene(pkg.cornell_box())
        here = plc.render_all(pkg, r)
    finally:
        r.close()
    # the ranges took hold: a forward-only launch writes 3 doubles per pixel and range and two count words per wave
    n_pixels = plc.W * plc.H
    per_range = n_pixels * 24 + (n_pixels + 63) // 64 * 8
    bytes_at = plc.STATS.index("path_bytes")
    for t in "AB":
        assert child[f"{t}/fwd/stats"][bytes_at] == 2 * per_range and here[f"{t}/fwd/stats"][bytes_at] == plc.SPP * per_range
    for k in ("fwd/image", "bwd/image", "bwd/grads"):
        assert child["A/" + k].tobytes() == child["B/" + k].tobytes(), k
    for t in "AB":
        for way in ("fwd", "bwd"):
            assert child[f"{t}/{way}/stats"][plc.STATS.index("path_launches")] == 1
            assert child[f"{t}/{way}/stats"][0] == here[f"{t}/{way}/stats"][0]                  # segments
            np.testing.assert_allclose(child[f"{t}/{way}/image"], here[f"{t}/{way}/image"], rtol=2e-5, atol=1e-7)
        ref = here[f"{t}/bwd/grads"]
        np.testing.assert_allclose(child[f"{t}/bwd/grads"], ref, rtol=2e-5, atol=1e-6 * np.abs(ref).max())
