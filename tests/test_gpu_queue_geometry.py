"""The queue wavefront (K1-K7: csrc/drt_kernels.h, drt_walk.h, drt_backward.h, drt_chain.h) with regions of MORE THAN ONE CHUNK, at small frames.

Every queue is cut into regions, one wave's share each, and the wave works through its region in chunks of 64 slots.  Almost all of the
route's bookkeeping sits in the step from one chunk to the next of the same region -- k_shade's `noff = off + DRT_WAVE` / `nw == w` branch,
the fill levels `running` / `run0` / `crun0` / `run1` / `crun1` / `n_cont` / `cand_running` carried over chunks, the prefetch of `nxt` from
the same region, `counts_next[w]` written only when the region ends, `chunk_slot` with region_shift - 6 > 0 in k_intersect, the
`for (off = begin; off < end; off += DRT_WAVE)` loops of K1, K6 and the chain kernels -- and shard_plan halves the region from 256 slots down
to 64 while a batch makes fewer than 32 regions per CU: on a 256-CU device every batch under 2^21 paths has regions of ONE chunk, which is
every other queue-route test with tight bounds.  A set DRT_HIP_REGION_SIZE is taken as given (csrc/drt_tuning.h, queue_region_shift;
tests/cpp/queue_regions_kat.cpp), and the settings are read once per process, so each row of ENVIRONMENTS is a child process
(tests/queue_child.py) that renders one fixed case list -- two frames (23 x 11 x 7 = 1771 paths, 9 x 5 x 7 = 315) x three tracers x four
analytic and three mesh scenes x the queue route forced three ways x forward, backward with an adjoint image, unbiased, loss_l2 and the
gradient image, f64 and f32, every render twice -- and writes every output into an .npz.  The children run one after the other, each at
most once; a child ends at its first error other than a refused gradient image, and after a child that ended with a nonzero status (a
signal, 134, 139, or the Python error a HIP error of a render becomes) or at its time limit no further child is started and every test
that needed one fails with that child's output.

Expected values are the fp64 restatement's (oracle.render), computed here on the CPU once per (scene, tracer, frame).  Bounds are the
project's stated ones, none new: f64 against the restatement 1e-9 of the largest component (+ 2^-24 of the largest value where the entry
point returns a float image) with equal segments and capped paths; f32: check_f32 of tests/test_gpu_parity.py, PIXEL_TOL with the flip
budget for the gradient image; every child against `default` 1e-9 in f64 with equal segments, capped paths and queue traffic (the queue
keeps the paths' order, so the counts may not move with the region size); r256_b600 against r256 1e-9.  A failure names environment, case,
field, index and -- for a pixel -- the region and chunk its first sample falls into.

Two things are by design and not compared: (1) the queue traffic of a mesh render under another DRT_HIP_TAIL_BOUNCES than `default`'s
(2 for the unbiased operator's rounds, else 1): a ray the second stage keeps in registers never sees a queue (k_shade, cont_row), so
r256_tail2's biased and r256_tail1's unbiased mesh renders are held to `default` in values, segments and capped paths only; (2) the
bits of a repeated gradient SUM over more than 8 parameters (params12): K6 adds those rows with LDS atomics in no fixed order
(drt_backward.h, GradAcc<R, 0>), so the child records the largest relative difference of its two renders' sums and the parent holds it
to 1e-12 in f64 and 1e-5 in f32, entry by entry, the rule of tests/test_gpu_mesh_geometry.py; everything else repeats bit for bit.

The last test renders one frame at the size where the plan chooses 256 slots by itself (512 x 512 at the smallest spp with more than
n_cu * 32 * 256 paths), in the pytest process with no setting, against k_path."""
import dataclasses
import math
import os
import shutil
import subprocess
import sys
import tempfile
import time
import types

import numpy as np
import pytest

import mesh_families as mf
import queue_child as qc
from test_gpu_launch_geometry import F32_EPS, Failures, lobe_conditioning, pixels_f32
from test_gpu_parity import PIXEL_TOL, check_f32

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64_TOL = 1e-9
ROUTE_IS_THE_CASES = {"DRT_HIP_MESH_PATH_MAX": "1073741824"}      # (tests/test_gpu_mesh_geometry.py) route choice is the case's, not the frame's
# name -> (settings, log2 of the region size the process renders with, paths per batch or 0)
ENVIRONMENTS = {
    "default": ({}, 6, 0),
    "r128": ({"DRT_HIP_REGION_SIZE": "128"}, 7, 0),
    "r256": ({"DRT_HIP_REGION_SIZE": "256"}, 8, 0),
    "r1024": ({"DRT_HIP_REGION_SIZE": "1024"}, 10, 0),
    "r256_b600": ({"DRT_HIP_REGION_SIZE": "256", "DRT_HIP_BATCH_PATHS": "600"}, 8, 600),
    "r256_tail2": ({"DRT_HIP_REGION_SIZE": "256", "DRT_HIP_TAIL_BOUNCES": "2"}, 8, 0),
    "r256_tail1": ({"DRT_HIP_REGION_SIZE": "256", "DRT_HIP_TAIL_BOUNCES": "1"}, 8, 0),
}
OTHERS = [e for e in ENVIRONMENTS if e != "default"]
SPECULAR = ("cornell_specular", "open_sheet")        # the scenes with a specular material that the frames' paths reach
# a child's time limit: four times the first `default` child.  Measured on an MI355X, from the process's start to its end: default 4.0 s
# (3.4 s of it between the context's creation and the last render: 2160 renders; nothing is compiled at run time on this route), r128 3.9,
# r256 3.9, r1024 4.4, r256_b600 6.3 (three batches per large frame), r256_tail2 4.0, r256_tail1 4.0 -> 16 s for `default` itself, and for
# every later child four times what the `default` child of THIS run took where that is more (a slower or busier machine)
CHILD_TIMEOUT = 16

_children = {}      # environment -> {key: array}, or the text of a child that failed
_stopped = None     # the output of the child after which no further child is started
_default_wall = None    # seconds the `default` child of this run took


def child(name):
    """environment `name`'s outputs; its child runs at most once, and none after one that failed in any way, crashed or hung"""
    global _stopped, _default_wall
    if name != "default" and "default" not in _children:
        child("default")      # (the control runs first: the later children's time limit comes from it)
    if name not in _children:
        if _stopped is not None:
            pytest.fail("no child is started after one that ended with a nonzero status, by a signal or at its time limit:\n" + _stopped)
        env = {k: v for k, v in os.environ.items() if not k.startswith("DRT_HIP_")}
        env.update(ROUTE_IS_THE_CASES)
        env.update(ENVIRONMENTS[name][0])
        limit = max(CHILD_TIMEOUT, 4.0 * (_default_wall or 0.0))
        d = tempfile.mkdtemp(prefix="drt_queue_child_")
        try:
            try:
                t0 = time.time()
                r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "queue_child.py"), d], capture_output=True, text=True, env=env,
                                   timeout=limit)
                wall = time.time() - t0
                text = f"child {name}: status {r.returncode}\n" + r.stdout[-3000:] + r.stderr[-3000:]
                if r.returncode != 0:       # a signal, 134, 139 -- or a Python error, which is how a HIP error of a render ends the child
                    _stopped = text
                if r.returncode == 0:
                    with np.load(os.path.join(d, "outputs.npz")) as z:
                        _children[name] = {k: z[k] for k in z.files}
                    if name == "default":
                        _default_wall = wall
                    print(f"child {name}: {wall:.1f} s, {float(_children[name]['seconds']):.1f} s of it rendering; "
                          f"refused: {sorted(set(k.split('/')[0] + ' ' + k.split('/')[4] + ' ' + str(v) for k, v in _children[name].items() if k.endswith('/refused'))) or 'nothing'}")
                else:
                    _children[name] = text
            except subprocess.TimeoutExpired as e:
                _stopped = _children[name] = f"child {name}: no end after {limit:.0f} s\n{e.stdout or ''}{e.stderr or ''}"[-6000:]
        finally:
            shutil.rmtree(d, ignore_errors=True)
    if isinstance(_children[name], str):
        pytest.fail(_children[name])
    return _children[name]


class Call:
    """one call's outputs of one child"""

    def __init__(self, outputs, name, tracer, frame, route, call, f64):
        self.outputs, self.where = outputs, (name, tracer, frame, route, call, f64)

    def has(self, field):
        return qc.key(*self.where, field) in self.outputs

    def get(self, field):
        return self.outputs[qc.key(*self.where, field)]

    def stat(self, field):
        return int(self.get("stats")[qc.STATS.index(field)])


def calls_of(outputs, name, tracer, frame, f64):
    return [Call(outputs, name, tracer, frame, route, call, f64) for route in qc.routes_for(name) for call in qc.CALLS]


# ---- where a value sits in the queue ------------------------------------------------------------------------------------------------
def batch_pixels(environment, frame):
    """pixels per batch, as shard_plan cuts the frame (csrc/drt_render_impl.h: Pb = batch paths / spp, every sample of a pixel in its batch)"""
    n_pixels, batch = frame[0] * frame[1], ENVIRONMENTS[environment][2]
    return min(max(batch // qc.SPP, 1), n_pixels) if batch else n_pixels


def locate(environment, frame, index):
    """the slot of a pixel's first sample at depth 0, where the queue still holds every path: path (s - s0) * Pb + (pixel - p0) of its batch"""
    if len(index) < 3:
        return f"row {tuple(int(i) for i in index)} of a sum over every region"
    shift = ENVIRONMENTS[environment][1]
    pixel = int(index[0]) * frame[0] + int(index[1])
    Pb = batch_pixels(environment, frame)
    i = pixel % Pb
    return (f"pixel (row {int(index[0])}, column {int(index[1])}) channel {int(index[2])}: first sample = path {i} of batch {pixel // Pb}, "
            f"region {i >> shift} (of {1 << shift} slots), chunk {(i & ((1 << shift) - 1)) >> 6}, lane {i & 63}")


def worst(got, want):
    d = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
    return np.unravel_index(int(np.argmax(d)), d.shape)


_worst = {}     # (environment, scene family) -> the worst f64 error against the restatement, of the largest component


def values_f64(environment, c, field, want, floats=False):
    """f64 mode against the restatement: F64_TOL of the largest component, + 2^-24 of it where the values came back as floats"""
    got = c.get(field)
    top = np.abs(want).max()
    err = np.abs(np.asarray(got, np.float64) - want).max() / top
    family = (environment, "mesh" if c.where[0] in qc.MESHES else "analytic")
    _worst[family] = max(_worst.get(family, 0.0), float(max(0.0, err - (F32_EPS if floats else 0.0))))
    assert top > 0 and err <= F64_TOL + (F32_EPS if floats else 0.0), \
        (environment, c.where, field, float(err), locate(environment, c.where[2], worst(got, want)))


# ---- the restatement's values: computed once per case, shared, never written to ----------------------------------------------------
_expected = {}


def expected(pkg, oracle, name, tracer, frame):
    where = (name, tracer, frame)
    if where in _expected:
        return _expected[where]
    scene, cam, rp = qc.scene_for(pkg, name), mf.camera(pkg, frame), qc.expected_params(pkg, name, tracer, frame)
    adjoint, target = qc.images(frame)
    E = {"scene": scene, "cam": cam, "rp": rp, "runs": []}

    def run(rp_=rp, **kw):
        r = oracle.render(scene, cam, rp_, **kw)
        E["runs"].append(r["stats"])
        return r
    fwd = run()
    E["image"], E["segments"] = fwd["image"], fwd["stats"]["segments"]
    E["capped"] = 0
    if rp.max_depth > 0:      # the run with the cap one vertex later tells which paths the cap cut (test_capped_paths_are_reported)
        E["capped"] = run(rp_=dataclasses.replace(rp, max_depth=rp.max_depth + 1))["stats"]["segments"] - E["segments"]
    E["grads"] = run(backward=True, adjoint=adjoint)["grads"]
    unb = run(backward=True, adjoint=adjoint, unbiased=True)
    E["unbiased"] = (unb["image"], unb["grads"], unb["stats"]["segments"])
    E["loss_l2"] = run(backward=True, adjoint=target, loss_l2=True)["grads"]
    E["gimg"] = run(backward=True, grad_image_param=qc.GIMG_PARAM)["grad_image"]
    for v in list(E.values()) + list(E["unbiased"]):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _expected[where] = E
    return E


# ---- 0: the inputs, on the CPU ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", qc.SCENES)
def test_inputs_stay_in_the_domain(pkg, oracle, name):
    """the conditions of tests/test_gpu_launch_geometry.py::test_inputs_stay_in_the_domain for this file's cases: the restatement draws no
    extreme number, goes no deeper than 40 vertices, has a nonzero largest gradient component under every operator and a nonzero gradient
    image, the capped tracer cuts paths -- and the restatement ALONE sets no pixel aside: in no scene, the meshes' specular faces
    included, does a pixel's specular lobe cost f32 more than the pixel bound (lobe_conditioning there), so the flip budget of the f32
    comparisons (one pixel per 100,000 paths) is left to paths that flip.  That the scenes of SPECULAR, and only they, have such a lobe
    at all shows that the vertices' flattened indices were mapped.  The seeds of queue_child.SEEDS are the first from 9 upwards at which
    all of this holds."""
    for tracer in range(len(qc.TRACERS)):
        for frame in qc.FRAMES:
            E = expected(pkg, oracle, name, tracer, frame)
            for st in E["runs"]:
                assert st["extreme_draws"] == 0 and st["deepest"] < 40, (name, tracer, frame, st)
            for g in (E["grads"], E["unbiased"][1], E["loss_l2"], E["gimg"]):
                assert np.abs(g).max() > 0 and np.isfinite(g).all(), (name, tracer, frame)
            assert (E["capped"] > 0) == (qc.TRACERS[tracer].get("max_depth", 0) > 0), (name, tracer, frame, E["capped"])
            # (mesh scenes too: the vertices name what they hit by its place in the flattened scene, a specular face of open_sheet included)
            kappa = lobe_conditioning(oracle, types.SimpleNamespace(scene=E["scene"], cam=E["cam"], rp=E["rp"]))
            assert (kappa.max() > 0) == (name in SPECULAR), (name, tracer, frame, float(kappa.max()))
            for v in (E["image"], E["gimg"]):
                lost = 4 * F32_EPS * kappa[..., None] * np.abs(v)
                assert lost.max() <= PIXEL_TOL * np.abs(v).max(), (name, tracer, frame, float(lost.max() / (PIXEL_TOL * np.abs(v).max())))


# ---- 1: the route, the batches, the refusals, the repeats --------------------------------------------------------------------------
def refused(c):
    """the status with which the library refused the call, None where it rendered; only the gradient image may be refused, so no
    comparison below passes over one of the other four calls"""
    status = str(c.get("refused")) if c.has("refused") else None
    assert status is None or (c.where[4] == "gimg" and status in qc.REFUSALS), (c.where, status)
    return status


@pytest.mark.parametrize("environment", ENVIRONMENTS)
def test_every_render_took_the_queue_route_and_repeats_bit_for_bit(environment):
    """no k_path launch, shade launches, k_intersect as a launch of its own exactly under DRT_RENDER_UNFUSED, the BVH walk exactly in mesh
    scenes; the batches the environment asks for; the library refuses nothing but a gradient image, and that with the same status in
    every process; and the second render of every call gave the first one's bits -- but params12's gradient sums over more than 8
    parameters (the docstring, (2)), whose two renders agree entry by entry within 1e-12 in f64 and 1e-5 in f32"""
    out, base = child(environment), child("default")
    assert set(out) == set(base)
    n, n_loose, worst_repeat = 0, 0, {True: 0.0, False: 0.0}
    for name, tracer, frame in qc.cases():
        n_batches = math.ceil(frame[0] * frame[1] / batch_pixels(environment, frame))
        for f64 in (True, False):
            for c in calls_of(out, name, tracer, frame, f64):
                assert refused(c) == refused(Call(base, *c.where)), (environment, c.where, refused(c))
                if refused(c):      # (the gradient image alone: refused())
                    continue
                n += 1
                assert c.stat("path_launches") == 0 and c.stat("shade_launches") > 0, (environment, c.where)
                assert (c.stat("intersect_launches") > 0) == (c.where[3] == "unfused"), (environment, c.where)
                assert (c.stat("walk_launches") > 0) == (name in qc.MESHES), (environment, c.where)
                assert c.stat("batches") == n_batches, (environment, c.where, c.stat("batches"), n_batches)
                moved = [str(f) for f in c.get("repeat")]
                if name == "params12" and "grads" in moved:     # sums over more than 8 parameters: tests/test_gpu_mesh_geometry.py's rule
                    moved.remove("grads")
                    n_loose += 1
                    worst_repeat[f64] = max(worst_repeat[f64], float(c.get("repeat_grads")))
                    assert float(c.get("repeat_grads")) <= (1e-12 if f64 else 1e-5), (environment, c.where, float(c.get("repeat_grads")))
                assert not moved, (environment, c.where, "the second render differs in", moved)
    assert n > 0
    print(f"{environment}: {n} calls rendered twice; params12's gradient sums moved in {n_loose} of them, by at most "
          f"{worst_repeat[True]:.2e} in f64 and {worst_repeat[False]:.2e} in f32")
    if environment == "r256_b600":
        assert batch_pixels(environment, qc.FRAMES[0]) * qc.SPP == 595


# ---- 2: against the restatement --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", qc.SCENES)
@pytest.mark.parametrize("environment", ENVIRONMENTS)
def test_f64_against_the_restatement(pkg, oracle, environment, name):
    out = child(environment)
    for tracer in range(len(qc.TRACERS)):
        for frame in qc.FRAMES:
            E = expected(pkg, oracle, name, tracer, frame)
            uimg, ugrads, usegments = E["unbiased"]
            for c in calls_of(out, name, tracer, frame, True):
                if refused(c):
                    continue
                call = c.where[4]
                want_segments = usegments if call == "unbiased" else E["segments"]
                assert c.stat("segments") == want_segments, (environment, c.where, c.stat("segments"), want_segments)
                if call != "unbiased":      # (the operator's suffixes are capped too: no restated count of those)
                    assert c.stat("capped_paths") == E["capped"], (environment, c.where, c.stat("capped_paths"), E["capped"])
                values_f64(environment, c, "image", uimg if call == "unbiased" else E["image"], floats=True)
                if call in ("bwd", "unbiased", "loss_l2"):
                    values_f64(environment, c, "grads", {"bwd": E["grads"], "unbiased": ugrads, "loss_l2": E["loss_l2"]}[call])
                if call == "gimg":
                    values_f64(environment, c, "gimg", E["gimg"], floats=True)
    family = (environment, "mesh" if name in qc.MESHES else "analytic")
    print(f"{environment} {name}: worst f64 error of {family[1]} scenes so far {_worst.get(family, 0.0):.3e}")


def with_location(environment, c, got, want):
    """the text a failed f32 comparison carries: where its worst value sits"""
    return f"worst at {locate(environment, c.where[2], worst(got, want))}"


@pytest.mark.parametrize("name", qc.SCENES)
@pytest.mark.parametrize("environment", ENVIRONMENTS)
def test_f32_against_the_restatement(pkg, oracle, environment, name):
    """check_f32 of tests/test_gpu_parity.py (flip-aware: at most one pixel per 100,000 paths set aside) for image and gradients, PIXEL_TOL
    with the same budget for the gradient image"""
    out = child(environment)
    failures = Failures()
    for tracer in range(len(qc.TRACERS)):
        for frame in qc.FRAMES:
            E = expected(pkg, oracle, name, tracer, frame)
            uimg, ugrads, usegments = E["unbiased"]
            n_paths = frame[0] * frame[1] * qc.SPP
            for c in calls_of(out, name, tracer, frame, False):
                if refused(c):
                    continue
                call = c.where[4]
                image, segments = (uimg, usegments) if call == "unbiased" else (E["image"], E["segments"])
                grads = {"bwd": E["grads"], "unbiased": ugrads, "loss_l2": E["loss_l2"]}.get(call)
                with failures.case(environment, *c.where, with_location(environment, c, c.get("image"), image)):
                    check_f32(c.get("image"), c.get("grads") if grads is not None else None, c.stat("segments"), image, grads, segments, n_paths=n_paths)
                if call == "gimg":
                    with failures.case(environment, *c.where, "gimg", with_location(environment, c, c.get("gimg"), E["gimg"])):
                        pixels_f32(c.get("gimg"), E["gimg"], n_paths, (environment,) + c.where)
    failures.raise_all()


# ---- 3: process against process --------------------------------------------------------------------------------------------------
def same_tail_as_default(environment, name, call):
    """whether the process renders the call's shade launches in as many stages as `default` does (the docstring, (1))"""
    if name not in qc.MESHES or "tail" not in environment:
        return True
    return (environment == "r256_tail2") == (call == "unbiased")


def against(environment, other, counts):
    out, base = child(environment), child(other)
    assert set(out) == set(base)
    top, n_same, n_all = 0.0, 0, 0
    for k in sorted(base):
        parts = k.split("/")
        if len(parts) != 7 or parts[5] != "f64" or parts[6] in ("repeat", "repeat_grads", "refused"):
            continue
        name, tracer, frame, route, call, _, field = parts
        a, b = out[k], base[k]
        if field == "stats":
            for s in counts:
                if s.startswith("queue_rays") and not same_tail_as_default(environment, name, call):
                    continue
                assert a[qc.STATS.index(s)] == b[qc.STATS.index(s)], (environment, other, k, s, int(a[qc.STATS.index(s)]), int(b[qc.STATS.index(s)]))
            continue
        n_all += 1
        n_same += int(np.array_equal(a, b))
        err = np.abs(a.astype(np.float64) - b.astype(np.float64)).max() / max(np.abs(b).max(), 1e-300)
        top = max(top, float(err))
        w, h = (int(v) for v in frame.split("x"))
        # (+ 2^-24 where the entry point returns floats: two fp64 sums 1e-15 apart may round to neighbouring floats)
        assert err <= F64_TOL + (F32_EPS if a.dtype == np.float32 else 0.0), (environment, other, k, float(err), locate(environment, (w, h), worst(a, b)))
    print(f"{environment} against {other}: worst f64 deviation {top:.2e}, {n_same} of {n_all} outputs bit-identical, child {float(out['seconds']):.1f} s")


@pytest.mark.parametrize("environment", OTHERS)
def test_f64_against_the_default_process(environment):
    """every f64 output within 1e-9 of the largest value of the `default` process's (regions of one chunk); segments, capped paths and the
    rays read from and written to the queues equal"""
    against(environment, "default", ("segments", "capped_paths", "queue_rays_read", "queue_rays_written"))


def test_batches_of_595_paths_against_the_whole_frame():
    """r256_b600 (23 x 11: three batches of 85 pixels x 7 samples = regions of 256 + 256 + 83 slots, the last batch 83 pixels; every
    batch accumulates into the same image and sums) against r256"""
    against("r256_b600", "r256", ("segments", "capped_paths", "queue_rays_read", "queue_rays_written"))


# ---- 4: the size at which the plan chooses 256 slots by itself ----------------------------------------------------------------------
_n_cu = []


def compute_units():
    """torch.cuda.get_device_properties(0).multi_processor_count, asked once and in a process of its own, so that this process holds one
    HIP runtime, the library's, as every other test of the suite does"""
    if not _n_cu:
        r = subprocess.run([sys.executable, "-c", "import torch; print('CUs', torch.cuda.get_device_properties(0).multi_processor_count)"],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "CUs" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
        _n_cu.append(int(r.stdout.split("CUs")[-1].split()[0]))
    return _n_cu[0]


@pytest.mark.parametrize("unbiased", [False, True])
def test_regions_of_256_slots_as_the_plan_chooses_them(pkg, hip, unbiased):
    """512 x 512 at the smallest spp with more than n_cu * 32 * 256 paths (9 on 256 CUs), no setting: the queue route with one launch per
    bounce against k_path, cornell at fixed depth 4, f64 -- 1e-9 of the largest component, equal segments.  No restatement at this size."""
    n_cu = compute_units()
    spp = (n_cu * 32 * 256) // (512 * 512) + 1
    assert 512 * 512 * spp > n_cu * 32 * 256 >= 512 * 512 * (spp - 1)
    hip.upload_scene(pkg.scene_by_name("cornell"))
    cam = pkg.cornell_camera(512, 512)
    rp = pkg.RenderParams(spp=spp, seed=9, **qc.TRACERS[0])
    img0, g0, st0 = hip.render(cam, rp, backward=True, unbiased=unbiased, f64=True)
    img1, g1, st1 = hip.render(cam, dataclasses.replace(rp, bounces_per_launch=1), backward=True, unbiased=unbiased, f64=True)
    assert st0["kernels"]["path"]["launches"] == 1 and st0["kernels"]["shade"]["launches"] == 0
    assert st1["kernels"]["path"]["launches"] == 0 and st1["kernels"]["shade"]["launches"] > 0 and st1["batches"] == 1
    g_err = float(np.abs(g1 - g0).max() / np.abs(g0).max())
    i_err = float(np.abs(img1.astype(np.float64) - img0).max() / np.abs(img0).max())
    print(f"{n_cu} CUs, {spp} spp, unbiased {unbiased}: segments {st1['segments']} / {st0['segments']}, gradients {g_err:.2e}, image {i_err:.2e}")
    assert st1["segments"] == st0["segments"] and st1["capped_paths"] == st0["capped_paths"]
    assert g_err <= F64_TOL and i_err <= F64_TOL + F32_EPS, (g_err, i_err, worst(img1, img0))
