"""The two device BVH walks -- k_intersect_mesh (csrc/drt_walk.h) and the walk inside k_path_mesh (csrc/drt_path_mesh.h) -- on geometry that
is not a closed sphere: tests/mesh_families.py.  Coincident faces (every hit an exact tie; traversal stacks deeper than the entries
k_path_mesh keeps in LDS, so its global overflow area runs), slivers with degenerate faces, an open sheet met from behind, meshes that
emit, two meshes around the analytic shapes, the build at the stack bound.  tests/test_mesh_families.py holds, on the CPU, that these
inputs are what they claim to be.

The expected values are the fp64 restatement's (oracle/drt_oracle.c: a linear scan over every triangle, no BVH to share a bug with).
f64: its segment count exactly, no capped path, gradients to 1e-9, image to f32 rounding; the two routes walk the same rays.
f32: gradients within 1e-4 of the restatement and of the other route, every pixel within 2e-4 of the largest but at most one.

The slivers decide hit or miss within f32 rounding of an edge, so they might flip more paths than the pixel rule allows.  Measured on
the first GPU run: 0 flipped pixels and f32 segment counts equal to the restatement's in every sliver render (24 x 20 x 2 under both
tracers and both routes, in batches of 257 and as a shard; 64 x 48 x 4 with per-face albedos; unbiased at 1 spp; 23 x 11 and 9 x 5 at 3 spp
in the three children) -- as in all 200 f32 comparisons of this file.  So the sliver cases keep the f32 rule of every other family.

The knobs of the mesh routes (csrc/drt_tuning.h: MESH_SHADE_MIN, BVH_DESCEND_MIN, BVH_REFILL, SHADE_LIST_GROUP, MESH_BLOCKS_PER_CU) are read once
per process: tests/mesh_child.py renders its case list in a process per setting (ENVIRONMENTS), and every child is compared with the
restatement and with the `default` child.  First run: each child makes its 96 renders in 0.5 s (mesh scenes compile nothing at run time),
under a second with the interpreter's start; `narrow` and `wide` differ from `default` in no bit of any f64 output."""
import dataclasses
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import mesh_child as mc
import mesh_families as mf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64_GRAD_TOL = 1e-9
F32_GRAD_TOL = 1e-4
F32_PIXEL_TOL = 2e-4
F32_SEGMENTS = 8                 # tests/test_gpu_mesh.py: one flipped path's length


def grad_rel_err(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


# ---- the restatement's values: computed once per case, shared, never written to --------------------------------------------------------
_reference = {}


def reference(pkg, oracle, name, cam, rp, unbiased=False):
    k = (name, cam.width, cam.height, rp.spp, rp.seed, rp.min_bounces, rp.absorb, rp.shard, rp.n_shards, rp.band_rows, unbiased)
    if k not in _reference:
        scene = mc.scene_for(pkg, name)
        ref = oracle.render(scene, cam, dataclasses.replace(rp, batch_paths=0, bounces_per_launch=0), backward=True, unbiased=unbiased, zero_dir_miss=unbiased)
        for a in (ref["image"], ref["grads"]):
            a.setflags(write=False)
        _reference[k] = ref
    return _reference[k]


def assert_route(st, route):
    """which kernels ran: the one-launch k_path_mesh, or the queue wavefront with its walk kernel"""
    if route == "path":
        assert st["kernels"]["path"]["launches"] == st["batches"] and st["kernels"]["shade"]["launches"] == 0 and st["kernels"]["intersect_mesh"]["launches"] == 0
    else:
        assert st["kernels"]["path"]["launches"] == 0 and st["kernels"]["intersect_mesh"]["launches"] > 0


def check_f64(what, img, grads, segments, capped, ref):
    err = grad_rel_err(grads, ref["grads"])
    print(f"{what} f64: segments {segments} / {ref['stats']['segments']}, capped {capped}, gradient error {err:.2e}, "
          f"image error {float(np.abs(img.astype(np.float64) - ref['image']).max() / np.abs(ref['image']).max()):.2e}")
    assert segments == ref["stats"]["segments"] and capped == 0        # (no case sets a depth cap: the restatement caps no path either)
    assert err < F64_GRAD_TOL
    np.testing.assert_allclose(img, ref["image"].astype(np.float32), rtol=2e-7, atol=1e-12)


def check_f32(what, img, grads, segments, ref, other_grads=None):
    scale = np.abs(ref["image"]).max()
    bad = np.abs(img.astype(np.float64) - ref["image"]).max(-1) > F32_PIXEL_TOL * scale
    err = grad_rel_err(grads, ref["grads"])
    print(f"{what} f32: segments {segments - ref['stats']['segments']:+d}, pixels outside the bound {int(bad.sum())}, gradient error {err:.2e}"
          + (f", route against route {grad_rel_err(grads, other_grads):.2e}" if other_grads is not None else ""))
    assert np.isfinite(img).all() and np.isfinite(grads).all()
    assert abs(segments - ref["stats"]["segments"]) <= F32_SEGMENTS
    assert err <= F32_GRAD_TOL and (other_grads is None or grad_rel_err(grads, other_grads) <= F32_GRAD_TOL)
    assert bad.sum() <= 1            # (one pixel may hold an f32-flipped path: tests/test_gpu_parity.py)


def check_about(name, scene, grads, ref):
    """a parameter whose faces never win a tie gets exactly nothing, on the device as in the restatement; the others are reached wherever
    the restatement reaches them (on every whole frame: tests/test_mesh_families.py; a shard's rows may see nothing of them)"""
    reached, untouched = mf.ABOUT.get(name, ((), ()))
    for p in reached:
        i = scene.param_names.index(p)
        assert grads[i].any() == ref["grads"][i].any(), (p, grads[i], ref["grads"][i])
    for p in untouched:
        assert not grads[scene.param_names.index(p)].any(), (p, grads[scene.param_names.index(p)])


def fixed_order(scene):
    """the gradient sums run in a fixed order: up to 4 parameters (beyond: the general form's per-wave tables, LDS atomics)"""
    return scene.n_params <= 4


def render_both_routes(pkg, hip, oracle, name, cam, rp, label):
    """one case through k_path_mesh and through the queue route, f64 and f32, each twice (the same bits), against the restatement"""
    scene = mf.family(pkg, name)
    ref = reference(pkg, oracle, name, cam, rp)
    hip.upload_scene(scene)
    out = {}
    for f64 in (True, False):
        for route in ("path", "queue"):
            r = dataclasses.replace(rp, bounces_per_launch=1 if route == "queue" else 0)
            img, g, st = hip.render(cam, r, backward=True, f64=f64)
            img2, g2, _ = hip.render(cam, r, backward=True, f64=f64)
            assert_route(st, route)
            np.testing.assert_array_equal(img, img2)
            if fixed_order(scene):
                np.testing.assert_array_equal(g, g2)
            else:
                np.testing.assert_allclose(g, g2, rtol=1e-12 if f64 else 1e-5, atol=0)
            out[route, f64] = (img, g, st)
        (ip, gp, sp), (iq, gq, sq) = out["path", f64], out["queue", f64]
        for route, (img, g, st) in (("path", out["path", f64]), ("queue", out["queue", f64])):
            what = f"{label} {route}"
            if f64:
                check_f64(what, img, g, st["segments"], st["capped_paths"], ref)
            else:
                check_f32(what, img, g, st["segments"], ref, gq if route == "path" else gp)
            check_about(name, scene, g, ref)
        if f64:
            assert sp["segments"] == sq["segments"] and sp["capped_paths"] == sq["capped_paths"]
            assert sp["kernels"]["intersect_mesh"]["units"] == sq["kernels"]["intersect_mesh"]["units"]       # rays that reach the mesh bounds
    return out


@pytest.mark.parametrize("tracer", range(len(mf.TRACERS)))
@pytest.mark.parametrize("name", mf.BASE)
def test_family_against_the_restatement_on_both_routes(pkg, hip, oracle, name, tracer):
    render_both_routes(pkg, hip, oracle, name, mf.camera(pkg), mf.render_params(pkg, tracer), f"{name} tracer {tracer}")


@pytest.mark.parametrize("tracer", range(len(mf.TRACERS)))
@pytest.mark.parametrize("name", mf.OVERFLOW)
def test_overflow_families_in_batches_and_as_a_shard(pkg, hip, oracle, name, tracer):
    """k_path_mesh's overflow area is indexed by the thread of the GRID: a second batch and a shard are where a stride goes wrong"""
    cam = mf.camera(pkg)
    rp = mf.render_params(pkg, tracer, batch_paths=257)
    out = render_both_routes(pkg, hip, oracle, name, cam, rp, f"{name} tracer {tracer} batches of 257")
    assert out["path", True][2]["batches"] > 1 and out["queue", True][2]["batches"] > 1
    shard = dataclasses.replace(rp, shard=1, n_shards=3, band_rows=4)
    out = render_both_routes(pkg, hip, oracle, name, cam, shard, f"{name} tracer {tracer} shard 1 of 3 in batches of 257")
    rows = pkg.shard_rows(cam.height, 4, 3, 1)
    others = np.setdiff1d(np.arange(cam.height), rows)
    assert 0 < len(rows) < cam.height and not out["path", True][0][others].any()


@pytest.mark.parametrize("name", mf.UNBIASED)
def test_unbiased_operator_on_coincident_faces_and_slivers(pkg, hip, oracle, name):
    """the unbiased operator keeps the queue route (its rounds are k_intersect_mesh launches); 1 spp"""
    scene = mf.family(pkg, name)
    cam = mf.camera(pkg)
    rp = mf.render_params(pkg, mf.UNBIASED_TRACER, spp=1, seed=mf.UNBIASED_SEED)
    ref = reference(pkg, oracle, name, cam, rp, unbiased=True)
    hip.upload_scene(scene)
    for f64 in (True, False):
        img, g, st = hip.render(cam, rp, backward=True, unbiased=True, f64=f64)
        img2, _, _ = hip.render(cam, rp, backward=True, unbiased=True, f64=f64)
        assert_route(st, "queue")
        np.testing.assert_array_equal(img, img2)
        if f64:
            check_f64(f"{name} unbiased", img, g, st["segments"], st["capped_paths"], ref)
        else:
            check_f32(f"{name} unbiased", img, g, st["segments"], ref)
        check_about(name, scene, g, ref)


def test_per_face_parameters_on_slivers_share_the_overflow_allocation(pkg, hip, oracle):
    """12 face albedos + the 4 Cornell parameters = 16: the general gradient form, whose history column lies behind the traversal stacks'
    overflow area in ONE allocation (drt_render_impl.h, path_batch) -- on rays that do overflow.  Both routes accept the scene."""
    scene = mf.family(pkg, "slivers_faces")
    assert scene.n_params == 16
    for tracer in range(len(mf.TRACERS)):
        out = render_both_routes(pkg, hip, oracle, "slivers_faces", mf.camera(pkg, mf.FACES_FRAME), mf.render_params(pkg, tracer, spp=mf.FACES_SPP),
                                 f"slivers_faces tracer {tracer}")
        assert np.abs(out["path", True][1][4:]).max(1).min() > 0        # every face albedo is reached


@pytest.mark.parametrize("tracer", range(len(mf.TRACERS)))
def test_which_copy_of_a_deck_is_coloured_shows_only_where_paths_meet_it(pkg, hip, oracle, tracer):
    """`deck` (the odd-coloured copy first: it wins every tie) and `deck_last` (it never wins): the two frames are equal bit for bit in
    every pixel none of whose paths meets the mesh, and differ where the camera sees it.  (Pixels whose paths meet the mesh at a later
    vertex differ too: they carry the winning copy's colour.  Which pixels those are: the restatement's vertices.)"""
    cam = mf.camera(pkg)
    rp = mf.render_params(pkg, tracer)
    scene = mf.family(pkg, "deck")
    n_paths = cam.width * cam.height * rp.spp
    v = oracle.render(scene, cam, rp, dump_paths=n_paths)["vertices"]
    _, flats, _ = mf.flat_triangles(scene)
    on_mesh = np.isin(v[:, 8].astype(np.int64), flats)
    meets = np.zeros(cam.width * cam.height, dtype=bool)
    meets[(v[on_mesh, 0].astype(np.int64)) // rp.spp] = True
    first = np.zeros_like(meets)
    first[(v[on_mesh & (v[:, 1] == 0), 0].astype(np.int64)) // rp.spp] = True
    meets, first = meets.reshape(cam.height, cam.width), first.reshape(cam.height, cam.width)
    assert first.sum() >= 40 and (~meets).sum() >= 100
    for route in ("path", "queue"):
        r = dataclasses.replace(rp, bounces_per_launch=1 if route == "queue" else 0)
        for f64 in (True, False):
            hip.upload_scene(scene)
            a, _, _ = hip.render(cam, r, backward=True, f64=f64)
            hip.upload_scene(mf.family(pkg, "deck_last"))
            b, _, _ = hip.render(cam, r, backward=True, f64=f64)
            np.testing.assert_array_equal(a[~meets], b[~meets])
            assert (a[first] != b[first]).any()


# ---- the knobs of the mesh routes: a process per setting -----------------------------------------------------------------------------
ROUTE_IS_THE_CASES = {"DRT_HIP_MESH_PATH_MAX": "1073741824"}      # route choice is the case's (bounces_per_launch), not the frame's
ENVIRONMENTS = {
    "default": {},
    "narrow": {"DRT_HIP_MESH_SHADE_MIN": "1", "DRT_HIP_BVH_DESCEND_MIN": "1", "DRT_HIP_BVH_REFILL": "1", "DRT_HIP_SHADE_LIST_GROUP": "1",
               "DRT_HIP_MESH_BLOCKS_PER_CU": "1"},
    "wide": {"DRT_HIP_MESH_SHADE_MIN": "64", "DRT_HIP_BVH_DESCEND_MIN": "64", "DRT_HIP_BVH_REFILL": "64", "DRT_HIP_SHADE_LIST_GROUP": "64"},
}
# a child's time limit: the children of the first run took under a second each (above); a minute, for a machine under load
CHILD_TIMEOUT = 60

_children = {}      # environment -> {key: array}, or the text of a child that failed
_stopped = None     # the output of the child after which no further child is started


def child(name):
    """environment `name`'s outputs; its child runs at most once, and none after one that crashed or hung"""
    global _stopped
    if name not in _children:
        if _stopped is not None:
            pytest.fail("no child is started after one that ended by a signal or at its time limit:\n" + _stopped)
        env = {k: v for k, v in os.environ.items() if not k.startswith("DRT_HIP_")}
        env.update(ROUTE_IS_THE_CASES)
        env.update(ENVIRONMENTS[name])
        d = tempfile.mkdtemp(prefix="drt_mesh_child_")
        try:
            try:
                r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mesh_child.py"), d], capture_output=True, text=True, env=env,
                                   timeout=CHILD_TIMEOUT)
                text = f"child {name}: status {r.returncode}\n" + r.stdout[-3000:] + r.stderr[-3000:]
                if r.returncode < 0 or r.returncode in (134, 139):
                    _stopped = text
                if r.returncode == 0:
                    with np.load(os.path.join(d, "outputs.npz")) as z:
                        _children[name] = {k: z[k] for k in z.files}
                    print(f"child {name}: {float(_children[name]['seconds']):.1f} s")
                else:
                    _children[name] = text
            except subprocess.TimeoutExpired as e:
                _stopped = _children[name] = f"child {name}: no end after {CHILD_TIMEOUT} s\n{e.stdout or ''}{e.stderr or ''}"[-6000:]
        finally:
            shutil.rmtree(d, ignore_errors=True)
    if isinstance(_children[name], str):
        pytest.fail(_children[name])
    return _children[name]


def stat(c, name, tracer, frame, route, f64, field):
    return int(c[mc.key(name, tracer, frame, route, f64, "stats")][mc.STATS.index(field)])


@pytest.mark.parametrize("name", mc.SCENES)
@pytest.mark.parametrize("environment", ENVIRONMENTS)
def test_knobs_change_no_result(pkg, oracle, environment, name):
    """every setting against the restatement, by the bounds above, on both routes, whole and in batches of 257"""
    c = child(environment)
    for _, tracer, frame in [x for x in mc.cases() if x[0] == name]:
        cam = mf.camera(pkg, frame)
        for route in mc.routes_for(frame):
            rp = mc.render_params(pkg, tracer, route)
            ref = reference(pkg, oracle, name, cam, rp)
            other = route.replace("path", "queue") if route.startswith("path") else route.replace("queue", "path")
            what = f"{environment}: {name} tracer {tracer} {frame[0]}x{frame[1]} {route}"
            for f64 in (True, False):
                img, g = c[mc.key(name, tracer, frame, route, f64, "image")], c[mc.key(name, tracer, frame, route, f64, "grads")]
                s = lambda field, r=route: stat(c, name, tracer, frame, r, f64, field)
                if route.startswith("path"):
                    assert s("path_launches") == s("batches") and s("walk_launches") == 0
                else:
                    assert s("path_launches") == 0 and s("walk_launches") > 0
                assert s("batches") > 1 if route.endswith("batched") else s("batches") == 1
                if f64:
                    check_f64(what, img, g, s("segments"), s("capped_paths"), ref)
                    assert s("walked") == s("walked", other)
                else:
                    check_f32(what, img, g, s("segments"), ref, c[mc.key(name, tracer, frame, other, f64, "grads")])


@pytest.mark.parametrize("environment", [e for e in ENVIRONMENTS if e != "default"])
def test_knobs_against_the_default_process(environment):
    """f64: within 1e-9 of the largest value of the default process's outputs; segments, capped paths and walked rays equal
    (the rules of tests/test_gpu_launch_geometry.py)"""
    c, d = child(environment), child("default")
    assert set(c) == set(d)
    worst = 0.0
    for k in sorted(c):
        if k.endswith("/stats"):
            for field in ("segments", "capped_paths", "walked", "batches", "path_launches"):
                i = mc.STATS.index(field)
                assert c[k][i] == d[k][i], (k, field, c[k][i], d[k][i])
        elif "/f64/" in k:
            err = float(np.abs(c[k].astype(np.float64) - d[k]).max() / np.abs(d[k]).max())
            worst = max(worst, err)
            assert err <= F64_GRAD_TOL, (k, err)
    print(f"{environment} against default: worst f64 deviation {worst:.2e}")
