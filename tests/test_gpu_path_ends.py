"""The ends of a path in k_path_lean (csrc/drt_path.h), for kernels whose intersection program is compiled in: the LAST vertex stands behind
the bounce loop and only asks whether the path ended on a pure light, and on which -- the host compiles the scene's light set in
(PathForm::lights) and the hit there is light_end_sig (csrc/drt_prog.h): the closest light, and whether any other shape wins against it.
The FIRST vertex keeps the loop's code (an eye-relative form of its hit was built and measured, profiles/r17_path_ends.txt, and not kept);
the cases that were written for it -- depth caps 1 and 2, eyes on a plane, off every axis and inside a sphere -- stay: at cap 1 the first
vertex IS the last, at cap 2 the loop runs once.

The oracle is the pair of tracers of tests/test_gpu_path_lean.py: A (absorb 1, min_bounces = d) takes k_path_lean; B (absorb 0.5,
min_bounces = d, max_depth = d) has a user cap and takes the unchanged k_path, which knows nothing about either end.  Same draws, same
paths: image, gradients and segment count must agree BYTE FOR BYTE -- no tolerance.  Which kernel ran is read from the stats first: one
path launch each, the program the plan chose, and capped_paths (A's cap is the roulette's: 0; B counts the paths its user cap cut short).

Frames are 64 x 48 at 6 spp; every scene is rendered once, by a module fixture, at all its depths."""
import dataclasses
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import path_ends_child as pec
from test_gpu_path_roles import room

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def assert_same_bits(a, b, backward, program, what):
    assert a[2]["kernels"]["path"]["launches"] == 1 and b[2]["kernels"]["path"]["launches"] == 1, what
    program_a, program_b = program if isinstance(program, tuple) else (program, program)
    assert a[2]["path_program"] == program_a and b[2]["path_program"] == program_b, (what, a[2]["path_program"], b[2]["path_program"])
    assert a[2]["capped_paths"] == 0 and b[2]["capped_paths"] > 0, (what, a[2]["capped_paths"], b[2]["capped_paths"])
    assert a[2]["segments"] == b[2]["segments"] and a[2]["segments"] > 0, (what, a[2]["segments"], b[2]["segments"])
    assert a[0].tobytes() == b[0].tobytes(), (what, float(np.abs(a[0] - b[0]).max()))
    if backward:
        assert a[1].tobytes() == b[1].tobytes(), (what, float(np.abs(a[1] - b[1]).max()))


SCENES = {
    # name: (scene, specialisation, the program the stats must name -- for A and B where they differ --, cameras)
    "cornell/never": (lambda pkg: pkg.cornell_box(), "never", "builtin", ("reference", "off_axis", "in_sphere")),
    "cornell/now": (lambda pkg: pkg.cornell_box(), "now", "builtin", ("reference",)),
    "cornell/generic": (lambda pkg: pkg.cornell_box(), "generic", "sorted", ("off_axis",)),
    "room/now": (lambda pkg: room(pkg, "plain"), "now", "specialised", ("reference", "off_axis")),
    "lights_first/now": (lambda pkg: pec.lights_scene(pkg, True), "now", "specialised", ("reference", "off_axis")),
    "twins_first/now": (lambda pkg: pec.lights_scene(pkg, False), "now", "specialised", ("reference", "off_axis")),
    "scatterer_last/now": (lambda pkg: pec.lights_scene(pkg, True, scatterer_last=True), "now", "specialised", ("reference", "off_axis")),
    # (the library's k_path_lean for the reference's kinds knows the reference's light: with another light set the render keeps the built-in
    #  kinds and runs k_path, as B does -- no wrong light set may reach the kernel)
    "cornell_two_lights/never": (lambda pkg: pec.cornell_two_lights(pkg), "never", "builtin", ("reference",)),
    "cornell_two_lights/now": (lambda pkg: pec.cornell_two_lights(pkg), "now", "builtin", ("reference",)),
}
_cache = {}


def rendered(pkg, name):
    """every (camera, depth, forward / backward) of one scene under both tracers, from ONE context (its hiprtc kernels are made once)"""
    if name not in _cache:
        make, mode, _, cams = SCENES[name]
        m = {"never": pkg.SPECIALISE_NEVER, "now": pkg.SPECIALISE_NOW, "generic": pkg.SPECIALISE_GENERIC}[mode]
        out = {}
        r = pkg.HipRenderer(0)
        try:
            r.set_specialisation(m)
            r.upload_scene(make(pkg))
            for cname in cams:
                for depth in pec.DEPTHS:
                    for backward in (False, True):
                        out[cname, depth, backward] = pec.render_pair(pkg, r, pec.cameras(pkg)[cname], depth, backward)
        finally:
            r.close()
        _cache[name] = out
    return _cache[name]


@pytest.mark.parametrize("backward", [False, True], ids=["fwd", "bwd"])
@pytest.mark.parametrize("depth", pec.DEPTHS)
@pytest.mark.parametrize("name", list(SCENES))
def test_both_ends_keep_every_bit(pkg, name, depth, backward):
    """depth caps 1 (the first vertex IS the last), 2 (one loop iteration before it), 3 and 6; eyes on the front plane, off every axis and
    inside a sphere; the library's kernel and hiprtc's; lights that are not last, of two kinds, several of them; exact ties in both orders"""
    program = SCENES[name][2]
    for cname in SCENES[name][3]:
        out = rendered(pkg, name)[cname, depth, backward]
        print(name, cname, depth, "bwd" if backward else "fwd", "segments", out["A"][2]["segments"], "capped", out["B"][2]["capped_paths"],
              "mean", float(out["A"][0].mean()))
        assert_same_bits(out["A"], out["B"], backward, program, (name, cname, depth, backward))
        assert (depth == 1 and cname == "in_sphere") or out["A"][0].max() > 0, (name, cname, depth)   # (inside the sphere the eye sees no light)


def test_the_twin_that_stands_first_wins_the_tie(pkg):
    """the two orders of the coincident pairs are different scenes: with the lights first the ceiling and the upper sphere shine, with their
    diffuse twins first they scatter -- so the tie goes by scene order, in k_path_lean exactly as in k_path (the test above)"""
    first = rendered(pkg, "lights_first/now")["reference", 1, False]["A"]
    second = rendered(pkg, "twins_first/now")["reference", 1, False]["A"]
    # the pixel at the middle of the top row looks at the upper pair (behind it: the ceiling pair), one vertex deep: emission 1 where the
    # light stands first, nothing where its diffuse twin does -- in every sample
    top = (0, pec.W // 2)
    assert (first[0][top] == 1.0).all() and (second[0][top] == 0.0).all(), (first[0][top], second[0][top])
    assert second[0].max() > 0                                                  # (the small light at the end still shines)


def test_a_scatterer_behind_every_light_at_a_lights_own_place_changes_nothing(pkg):
    """the small light's diffuse twin as the LAST shape of the scene: every hit on it ties with the light before it, which wins -- so the
    twelve-shape scene renders the eleven-shape scene's image, gradients and segments bit for bit, through its own kernel"""
    for cname in ("reference", "off_axis"):
        for depth in pec.DEPTHS:
            for backward in (False, True):
                a = rendered(pkg, "lights_first/now")[cname, depth, backward]["A"]
                b = rendered(pkg, "scatterer_last/now")[cname, depth, backward]["A"]
                assert a[2]["segments"] == b[2]["segments"] and a[0].tobytes() == b[0].tobytes(), (cname, depth, backward)
                if backward:
                    assert a[1].tobytes() == b[1].tobytes(), (cname, depth)


def test_the_kind_sorted_program_renders_what_the_compiled_in_one_does(pkg):
    """builtin == sorted, bit for bit, as before: the kind-sorted program keeps the loop as it was at both ends"""
    for depth in pec.DEPTHS:
        for backward in (False, True):
            a = rendered(pkg, "cornell/never")["off_axis", depth, backward]["A"]
            b = rendered(pkg, "cornell/generic")["off_axis", depth, backward]["A"]
            assert a[2]["path_program"] == "builtin" and b[2]["path_program"] == "sorted"
            assert a[2]["segments"] == b[2]["segments"] and a[0].tobytes() == b[0].tobytes(), (depth, backward)
            if backward:
                assert a[1].tobytes() == b[1].tobytes(), depth


@pytest.mark.parametrize("name,program", [("cornell", "builtin"), ("lights_first", "specialised")])
def test_a_shard_and_an_adjoint_image(pkg, name, program):
    """a shard that is not the whole frame (the second of two, bands of 16 rows), seeded with an adjoint image"""
    rng = np.random.default_rng(5)
    adjoint = rng.uniform(-1.0, 2.0, (pec.H, pec.W, 3)).astype(np.float32)
    r = pkg.HipRenderer(0)
    try:
        r.set_specialisation(pkg.SPECIALISE_NOW)
        r.upload_scene(pkg.cornell_box() if name == "cornell" else pec.lights_scene(pkg, True))
        for depth in (1, 3):
            out = pec.render_pair(pkg, r, pec.cameras(pkg)["off_axis"], depth, True, adjoint=adjoint, shard=1, n_shards=2, band_rows=16)
            assert_same_bits(out["A"], out["B"], True, program, (name, depth))
            rows = pkg.shard_rows(pec.H, 16, 2, 1)
            others = np.setdiff1d(np.arange(pec.H), rows)
            assert not out["A"][0][others].any()
            if depth > 1:                                                       # (one vertex deep the middle band may see no light)
                assert out["A"][0][rows].max() > 0
                whole = pec.render_pair(pkg, r, pec.cameras(pkg)["off_axis"], depth, True)["A"]
                assert out["A"][1].tobytes() != whole[1].tobytes()              # (the seed and the shard took hold)
    finally:
        r.close()


def test_sample_ranges_of_three_samples(pkg):
    """DRT_HIP_PATH_SPR = 3 in a child process: 6 spp in two ranges of 3 -- the sample loop runs the bounce loop and the last vertex behind it
    three times per wave.  A against B bit for bit there; against this process's one-sample ranges the image sums in another order."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("DRT_HIP_")}
    env["DRT_HIP_PATH_SPR"] = "3"
    d = tempfile.mkdtemp(prefix="drt_path_ends_")
    try:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "path_ends_child.py"), d], capture_output=True, text=True, env=env, timeout=240)
        assert p.returncode == 0, f"child: status {p.returncode}\n" + p.stdout[-3000:] + p.stderr[-3000:]
        with np.load(os.path.join(d, "outputs.npz")) as z:
            child = {k: z[k] for k in z.files}
    finally:
        shutil.rmtree(d, ignore_errors=True)
    n_pixels = pec.W * pec.H
    per_range = n_pixels * 24 + (n_pixels + 63) // 64 * 8      # a forward-only launch: 3 doubles per pixel and range, two count words per wave
    for cname in ("reference", "off_axis"):
        here = rendered(pkg, "cornell/never")
        for depth in (1, 2, 3):
            for backward in (False, True):
                tag = f"{cname}/{depth}/{'bwd' if backward else 'fwd'}"
                a, b = child[tag + "/A/stats"], child[tag + "/B/stats"]
                assert a[3] == 1 and b[3] == 1 and a[1] == 0 and b[1] > 0, (tag, a, b)
                assert a[0] == b[0] == here[cname, depth, backward]["A"][2]["segments"], tag
                if not backward:
                    assert a[2] == 2 * per_range and here[cname, depth, False]["A"][2]["path_bytes"] == pec.SPP * per_range, (tag, a[2])
                assert child[tag + "/A/image"].tobytes() == child[tag + "/B/image"].tobytes(), tag
                np.testing.assert_allclose(child[tag + "/A/image"], here[cname, depth, backward]["A"][0], rtol=2e-5, atol=1e-7)
                if backward:
                    assert child[tag + "/A/grads"].tobytes() == child[tag + "/B/grads"].tobytes(), tag


def one_launch_against_the_queue_route(pkg, scene, rp, mode):
    """scenes and renders that do not qualify keep k_path, in one launch: against the queue route within tests/test_gpu_path_lean.py's bounds"""
    cam = pec.cameras(pkg)["off_axis"]
    r = pkg.HipRenderer(0)
    try:
        r.set_specialisation(mode)
        r.upload_scene(scene)
        ref = r.render(cam, dataclasses.replace(rp, bounces_per_launch=1), backward=True)
        got = r.render(cam, rp, backward=True)
    finally:
        r.close()
    assert ref[2]["kernels"]["path"]["launches"] == 0 and got[2]["kernels"]["path"]["launches"] == 1
    assert abs(got[2]["segments"] - ref[2]["segments"]) <= 64
    np.testing.assert_allclose(got[0], ref[0], rtol=2e-5, atol=1e-7)
    np.testing.assert_allclose(got[1], ref[1], rtol=2e-5, atol=1e-6 * np.abs(ref[1]).max())
    return got


def test_a_wall_that_also_emits_keeps_k_path(pkg):
    scene = pkg.cornell_box(emissive_wall=True)
    got = one_launch_against_the_queue_route(pkg, scene, pkg.RenderParams(spp=pec.SPP, min_bounces=3, absorb=1.0, seed=pec.SEED), pkg.SPECIALISE_NEVER)
    assert got[2]["path_program"] == "builtin"


def test_a_roulette_inside_the_loop_keeps_k_path(pkg):
    got = one_launch_against_the_queue_route(pkg, pkg.cornell_box(), pkg.RenderParams(spp=pec.SPP, min_bounces=1, absorb=0.5, seed=pec.SEED), pkg.SPECIALISE_NEVER)
    assert got[2]["path_program"] == "builtin"
