"""Every k_path form at the launch geometry large frames get: sample ranges of SEVERAL samples, a short last range, one range per pixel
group, lanes that regenerate, and the general form's other layouts.

The one-launch path kernels split a frame as wave <-> (64 pixels, a range of `spr` samples); shard_plan sizes the ranges so that a 256-CU
device sees spr = 1 until a frame has ~1.8 M camera samples, far above every other test of the suite.  The DRT_HIP_* settings are read once
per process, so each geometry below is a child process (tests/geometry_child.py) that renders one fixed case list -- two frames (23 x 11:
three full pixel groups and one of 61 lanes; 9 x 5: 19 lanes without a pixel) x three tracers x six scenes x every entry point, f64 and
f32 -- and writes every output into an .npz.  The children run one after the other, each at most once (the module's cache); after a child
that ended by a signal, with status 134 or 139, or at its time limit no further child is started and every test that needed one fails
with that child's output.

Expected values are the fp64 restatement's (oracle.render), computed here on the CPU once per (scene, tracer, frame), never the device's:
image, gradients, segments and capped paths of the plain renders; the Jacobian as one gradient image per parameter and J v from it; A, b and
loss from those; set k's image, tangent and gradient from the restatement with P_k installed.  Two exceptions: the cross form's `bias` and
variance image (the restatement has no per-sample values: against the `default` child's; A, b + bias and loss + bias[K] against the
restated plain values) and the batched renders (against the same child's unbatched ones).

Bounds are the project's stated ones, none new: f64 against the restatement 1e-9 of the largest component (+ 2^-24 of the largest value
where the entry point returns a float image) with equal segments and capped paths, 1e-9 of the sum of absolute terms for reduced sums;
f32: check_f32 of tests/test_gpu_parity.py for image and gradients, PIXEL_TOL with test_gpu_tangent.py's flip budget for derivative images,
GRAD_TOL of the sum of absolute terms for sums; f64 between two geometries 1e-9.  Where two geometries agree bit for bit it is printed, not
asserted.

That DRT_HIP_PATH_REGEN=1 took effect cannot be read from the statistics (there is no such field); that the sample ranges took hold can,
and is asserted for every geometry: with spr back at 1 (the `default` row) those assertions fail for every other row.

Measured on an MI355X, three runs.  Each child's wall time, from the context's creation to its last render (3121 arrays of 36 cases): default
8.2 ... 15.7 s (the first child compiles the hiprtc kernels of cornell_disc_box and the f32 LOSS kernels; the later ones find them in ROCm's
on-disk cache), spr3 1.0, spr64 1.1, regen_eager 0.9, regen_lazy 0.9 ... 1.0, gen_small 2.2 ... 3.4, gen_wide 6.7 ... 7.0; the whole file
35 s.  Worst f64 error against the restatement: 2.5e-14 in every geometry (of the largest component / the sum of absolute terms).  Against
`default`, bit for bit in every geometry: the forward image, the gradient image, render_tangents' and render_normal_equations' outputs (float
images of fp64 sums, and the Jacobian form's sums); under spr64 also _along, the parameter sets and render_tangent.  Not bit-identical, all
within 1.7e-15 of the largest value: summed gradients (render backward, unbiased, loss_l2 in part, param_sets_grad everywhere), the double images of
render_tangent and the parameter sets and the sums formed from them, and the cross form's corrections -- the fp64 grouping moves."""
import dataclasses
import math
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import geometry_child as gc
from test_gpu_cross import close, plain, scales
from test_gpu_parity import FLIP_MIN_REL, GRAD_TOL, PIXEL_TOL, check_f32, flip_budget
from test_gpu_sets_grad import with_params
from test_gpu_tangents import sums_close

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64_TOL = 1e-9
F32_EPS = 2.0 ** -24

# name -> (environment, the forced samples per range or None)
GEOMETRIES = {
    "default": ({}, None),
    "spr3": ({"DRT_HIP_PATH_SPR": "3"}, 3),
    "spr64": ({"DRT_HIP_PATH_SPR": "64"}, 64),
    "regen_eager": ({"DRT_HIP_PATH_REGEN": "1", "DRT_HIP_PATH_SPR": "3", "DRT_HIP_PATH_REGEN_MIN": "1"}, 3),
    "regen_lazy": ({"DRT_HIP_PATH_REGEN": "1", "DRT_HIP_PATH_SPR": "5", "DRT_HIP_PATH_REGEN_MIN": "64"}, 5),
    "gen_small": ({"DRT_HIP_PATH_SPR": "3", "DRT_HIP_GEN_ABOVE": "0", "DRT_HIP_GEN_HIST_LDS": "0", "DRT_HIP_GEN_COPIES_LOG2": "0"}, 3),
    "gen_wide": ({"DRT_HIP_PATH_SPR": "3", "DRT_HIP_GEN_ABOVE": "8", "DRT_HIP_GEN_HIST_LDS": "16"}, 3),
}
OTHERS = [g for g in GEOMETRIES if g != "default"]
# a child's time limit: fifteen times the slowest child seen (15.7 s: `default`, the one that compiles; see the docstring), for a machine
# where every child compiles and more
CHILD_TIMEOUT = 240


# ---- the children ----------------------------------------------------------------------------------------------------------------
_children = {}      # geometry -> {key: array}, or the text of a child that failed
_stopped = None     # the output of the child after which no further child is started


def child(name):
    """geometry `name`'s outputs; its child runs at most once, and none after one that crashed or hung"""
    global _stopped
    if name not in _children:
        if _stopped is not None:
            pytest.fail("no child is started after one that ended by a signal or at its time limit:\n" + _stopped)
        env = {k: v for k, v in os.environ.items() if not k.startswith("DRT_HIP_")}
        env.update(GEOMETRIES[name][0])
        d = tempfile.mkdtemp(prefix="drt_geometry_")
        try:
            try:
                r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "geometry_child.py"), d], capture_output=True, text=True,
                                   env=env, timeout=CHILD_TIMEOUT)
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


def key(name, tracer, frame, call, f64, field):
    return f"{name}/{tracer}/{frame[0]}x{frame[1]}/{call}/{'f64' if f64 else 'f32'}/{field}"


class Case:
    """one case's outputs of one child"""

    def __init__(self, outputs, name, tracer, frame):
        self.outputs, self.where = outputs, (name, tracer, frame)

    def get(self, call, f64, field):
        return self.outputs[key(*self.where, call, f64, field)]

    def stat(self, call, f64, field):
        return int(self.get(call, f64, "stats")[gc.STATS.index(field)])


# ---- the restatement's values ----------------------------------------------------------------------------------------------------
_expected = {}


def jacobian(oracle, scene, cam, rp):
    """the restatement's gradient image of every parameter: with the default seed d L_c / d theta_{p,c} per pixel, [P, H, W, 3]"""
    return np.stack([np.array(oracle.render(scene, cam, rp, backward=True, grad_image_param=p)["grad_image"], dtype=np.float64)
                     for p in range(scene.n_params)])


def eq_terms(T, r):
    """the per-pixel terms of A [H,W,3,K,K], b [H,W,3,K] and the loss [H,W,3] from derivative images T [K,H,W,3] and a residual r [H,W,3]"""
    return {"A": np.einsum("khwc,lhwc->hwckl", T, T), "b": np.einsum("khwc,hwc->hwck", T, r), "loss": r * r}


def restated_terms(E, call):
    """the per-pixel terms [H,W,...] of every reduced sum of `call`, from the restatement's images"""
    target = E["x"].target.astype(np.float64)
    if call == "neq":
        return eq_terms(E["J"], E["image"] - target)
    if call in ("along", "cross"):
        return eq_terms(E["T"], E["image"] - target)
    if call == "cross2":
        return eq_terms(E["T2"], E["image2"] - target)
    n = 3 if call == "sets" else 2
    rk = E["set_images"][:n] - target
    terms = {"loss": rk * rk}
    if call == "sets_along":
        terms.update(dloss=2 * rk * E["set_tangents"], curv=E["set_tangents"] * E["set_tangents"])
    return {f: np.moveaxis(t, 0, 2) for f, t in terms.items()}


def expected(pkg, oracle, name, tracer, frame):
    """everything the restatement says about one case: computed once, read-only"""
    where = (name, tracer, frame)
    if where in _expected:
        return _expected[where]
    x = gc.inputs(pkg, name, tracer, frame)
    scene, cam, rp = x.scene, x.cam, x.rp
    E = {"x": x, "runs": []}

    def run(sc=scene, rp_=rp, **kw):
        r = oracle.render(sc, cam, rp_, **kw)
        E["runs"].append(r["stats"])
        return r
    fwd = run()
    E["image"], E["segments"] = fwd["image"], fwd["stats"]["segments"]
    E["capped"] = 0
    if rp.max_depth > 0:      # the run with the cap one vertex later tells which paths the cap cut (test_capped_paths_are_reported)
        E["capped"] = run(rp_=dataclasses.replace(rp, max_depth=rp.max_depth + 1))["stats"]["segments"] - E["segments"]
    E["grads"] = run(backward=True, adjoint=x.adjoint)["grads"]
    unb = run(backward=True, adjoint=x.adjoint, unbiased=True)
    E["unbiased"] = (unb["image"], unb["grads"], unb["stats"]["segments"])
    E["loss_l2"] = run(backward=True, adjoint=x.target, loss_l2=True)["grads"]
    E["gimg"] = run(backward=True, grad_image_param=x.gparam)["grad_image"]
    calls = gc.derived_calls(name)
    if calls:
        J = jacobian(oracle, scene, cam, rp)
        E["J"] = J
        E["T"] = np.einsum("phwc,kpc->khwc", J, x.V)
    if "cross2" in calls:
        E["image2"] = run(rp_=x.rp2)["image"]
        E["T2"] = np.einsum("phwc,kpc->khwc", jacobian(oracle, scene, cam, x.rp2), x.V)
    if "sets" in calls or "sets_grad" in calls:
        refs = [run(sc=with_params(scene, x.P[k]), backward=True, adjoint=x.W[k]) for k in range(3)]
        E["set_images"] = np.stack([r["image"] for r in refs])
        E["set_grads"] = np.stack([r["grads"] for r in refs])
    if "sets_along" in calls:
        E["set_tangents"] = np.stack([np.einsum("phwc,pc->hwc", jacobian(oracle, with_params(scene, x.P[k]), cam, rp), x.D[k]) for k in range(2)])
    for v in E.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _expected[where] = E
    return E


# ---- comparisons -----------------------------------------------------------------------------------------------------------------
_worst = {}     # geometry -> the worst f64 error against the restatement, of the largest component / the sum of absolute terms


def note(geometry, err):
    _worst[geometry] = max(_worst.get(geometry, 0.0), float(err))


def values_f64(geometry, got, want, what, floats=False):
    """f64 mode against the restatement: F64_TOL of the largest component, + 2^-24 of it where the values came back as floats"""
    top = np.abs(want).max()
    err = np.abs(np.asarray(got, np.float64) - want).max() / top
    note(geometry, max(0.0, err - (F32_EPS if floats else 0.0)))
    assert top > 0 and err <= F64_TOL + (F32_EPS if floats else 0.0), (what, err)


def sums_f64(geometry, got, terms, what):
    """a reduced sum against the sum of the restated per-pixel terms: F64_TOL of the sum of absolute terms"""
    want, scale = terms.sum((0, 1)), np.abs(terms).sum((0, 1))
    note(geometry, (np.abs(got - want) / np.maximum(scale, 1e-300)).max())
    sums_close(got, want, scale, F64_TOL, what)


class Failures:
    """the f32 tests go through every case and call before they fail: a report names all that are outside a bound, not the first"""

    def __init__(self):
        self.found = []

    def case(self, *what):
        return _FailureScope(self, what)

    def raise_all(self):
        assert not self.found, f"{len(self.found)} outside their bounds:\n" + "\n".join(self.found)


class _FailureScope:
    def __init__(self, owner, what):
        self.owner, self.what = owner, what

    def __enter__(self):
        return self

    def __exit__(self, kind, value, tb):
        if kind is not None and issubclass(kind, AssertionError):
            self.owner.found.append(f"{self.what}: {str(value)[:400]}")
            return True
        return False


def pixels_f32(got, want, n_paths, what):
    """an f32 derivative image against the restated one: PIXEL_TOL of the largest value, flip-aware exactly as
    tests/test_gpu_tangent.py::test_f32_per_pixel_against_f64 -> the pixels set aside [H,W]"""
    got = np.asarray(got, np.float64)
    d = np.abs(got - want).max(-1)
    bad = d > PIXEL_TOL * np.abs(want).max()
    assert bad.sum() <= flip_budget(n_paths), (what, int(bad.sum()), float(d.max() / np.abs(want).max()))
    if bad.any():
        own = np.maximum(np.abs(want)[bad].max(-1), np.abs(got)[bad].max(-1))
        assert (d[bad] >= FLIP_MIN_REL * own).all(), (what, "a set-aside pixel differs by a rounding-sized amount", (d[bad] / own).min())
    return bad


def sums_f32(got, terms_got, terms_want, aside, what):
    """an f32 reduced sum against the restated terms: GRAD_TOL of the sum of absolute terms once the set-aside pixels' share -- on the
    device's side as its own images give it -- is removed from both (tests/test_gpu_tangents.py::test_f32_per_pixel_against_f64)"""
    keep = ~aside
    err = np.abs((got - terms_got[aside].sum(0)) - terms_want[keep].sum(0))
    scale = np.abs(terms_want[keep]).sum(0)
    assert (err <= GRAD_TOL * scale + 1e-300).all(), (what, float((err / np.maximum(scale, 1e-300)).max()))


def plain_counts(c, E, call, f64):
    assert c.stat(call, f64, "segments") == E["segments"] and c.stat(call, f64, "capped_paths") == E["capped"], (call, c.where)


def flat_materials(scene):
    """the material of every entry of the flattened scene, in which the restatement's vertices name what they hit (oracle/drt_oracle.c,
    raycast: every triangle of a mesh counts as a shape): the face's own material where the mesh has one per face, else the shape's"""
    out, mesh = [], sys.modules[type(scene).__module__].SHAPE_MESH
    for t, m, _, p in scene.shapes:
        if t != mesh:
            out.append(m)
            continue
        _, indices, face_material = scene.meshes[int(p[0])]
        out.extend([m] * len(indices) if face_material is None else [int(f) for f in face_material])
    return out


def lobe_conditioning(oracle, x, max_vertices=0):
    """The f32 conditioning of the reference's specular lobe, per pixel [H,W]: the largest c^2 / (1 - c^2) over the specular bounces of the
    pixel's paths, c = normal . half vector, from the restatement's vertices.  The lobe's factor s = sqrt(1 - c^2) (bxdf.hpp:104-107) loses
    what 1 - c^2 cancels: a rounding of 2^-24 in c^2 is a relative 2^-24 c^2 / (1 - c^2) in s^2, and c (two normalisations and a dot
    product) carries a few roundings itself.  First seen on cornell_specular, depth 5, 23 x 11, seed 9: pixel (4, 11) is ONE path whose
    first half vector lies 5e-3 rad off the sphere's normal, c^2 / (1 - c^2) = 40969 -- every f32 geometry, `default` included, gives
    that pixel 0.54 % above the restatement, in the image and in every derivative image alike.
    max_vertices: room for the vertex log where the render is a shard of a large frame (tests/index_range.py); default 64 per path."""
    scene, cam, rp = x.scene, x.cam, x.rp
    specular = [i for i, m in enumerate(flat_materials(scene)) if m >= 0 and scene.materials[m][0] == 1]
    v = oracle.render(scene, cam, rp, dump_paths=cam.width * cam.height * rp.spp, max_vertices=max_vertices)["vertices"]
    v = v[np.lexsort((v[:, 1], v[:, 0]))]
    a, b = v[:-1], v[1:]                                  # a vertex and the next one of the same path: directions in and out
    on = (a[:, 0] == b[:, 0]) & (b[:, 1] == a[:, 1] + 1) & np.isin(a[:, 8].astype(int), specular)
    a, b = a[on], b[on]
    n = a[:, 13:16] / np.linalg.norm(a[:, 13:16], axis=1)[:, None]
    half = b[:, 5:8] - a[:, 5:8]
    half /= np.linalg.norm(half, axis=1)[:, None]
    c2 = np.square((n * half).sum(1))
    out = np.zeros(cam.width * cam.height)
    np.maximum.at(out, (a[:, 0] // rp.spp).astype(int), c2 / np.maximum(1 - c2, 1e-300))
    return out.reshape(cam.height, cam.width)


# ---- 0: the inputs, on the CPU ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", gc.SCENES)
def test_inputs_stay_in_the_domain(pkg, oracle, name):
    """for every (tracer, frame) of the scene the restatement draws no extreme number, goes no deeper than 40 vertices (beyond that host
    and device no longer stand on the same point: tools/fuzz_modes.py), has a nonzero largest gradient component under every operator and
    a nonzero gradient image, the capped tracer cuts paths, and no pixel's specular lobe is conditioned worse than the f32 pixel bound
    allows (lobe_conditioning).  The seeds of geometry_child.SEEDS are the first at which all of this holds."""
    for tracer in range(len(gc.TRACERS)):
        for frame in gc.FRAMES:
            E = expected(pkg, oracle, name, tracer, frame)
            for st in E["runs"]:
                assert st["extreme_draws"] == 0 and st["deepest"] < 40, (name, tracer, frame, st)
            for g in (E["grads"], E["unbiased"][1], E["loss_l2"], E["gimg"]):
                assert np.abs(g).max() > 0 and np.isfinite(g).all(), (name, tracer, frame)
            assert (E["capped"] > 0) == (gc.TRACERS[tracer].get("max_depth", 0) > 0), (name, tracer, frame, E["capped"])
            if "T" in E:
                assert all(np.abs(t).max() > 0 for t in E["T"])
            # ... and inside the f32 comparison's domain: no pixel whose specular lobe alone costs f32 more than the pixel bound -- four
            # roundings' worth of the cancellation in sqrt(1 - c^2), times the pixel's own value, against PIXEL_TOL of the largest value
            kappa = lobe_conditioning(oracle, E["x"])
            for v in [E["image"], E["gimg"]] + list(E.get("T", [])):
                lost = 4 * F32_EPS * kappa[..., None] * np.abs(v)
                assert lost.max() <= PIXEL_TOL * np.abs(v).max(), (name, tracer, frame, float(lost.max() / (PIXEL_TOL * np.abs(v).max())))


# ---- 1: the geometry took hold ---------------------------------------------------------------------------------------------------
def batch_layout(n_pixels, spp, batch_paths):
    """(pixels, samples) of every batch, as shard_plan and the batch loop of render_impl cut a frame"""
    Pb = min(max(batch_paths // spp, 1), n_pixels)
    Sb = max(min(batch_paths // Pb, spp), 1)
    return [(min(Pb, n_pixels - p0), min(Sb, spp - s0)) for p0 in range(0, n_pixels, Pb) for s0 in range(0, spp, Sb)]


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_the_sample_ranges_took_hold(geometry):
    """the ranges of every frame, from the forward-only renders' path_bytes: ceil(Sb / min(spr, Sb)) per batch under a forced spr -- and
    under `default` as many ranges as samples: the plan never leaves one sample per range at these sizes (the control: this is what every
    other test of the suite renders with)"""
    out = child(geometry)
    spr = GEOMETRIES[geometry][1] or 1
    for name, tracer, frame in gc.cases():
        c = Case(out, name, tracer, frame)
        n_pixels = frame[0] * frame[1]
        for f64 in (True, False):
            for call, spp in (("fwd", gc.SPP), ("fwd2", gc.SPP_CROSS)):
                assert c.stat(call, f64, "path_launches") == 1 and c.stat(call, f64, "shade_launches") == 0
                assert int(c.get(call, f64, "ranges")) == math.ceil(spp / min(spr, spp)), (geometry, c.where, call, int(c.get(call, f64, "ranges")))
            layout = batch_layout(n_pixels, gc.SPP, gc.BATCH_PATHS[frame])
            want = sum(math.ceil(Sb / min(spr, Sb)) * gc.forward_bytes_per_range(Pb) for Pb, Sb in layout)
            assert c.stat("fwd_batched", f64, "batches") == len(layout) > 1
            assert c.stat("fwd_batched", f64, "path_launches") == len(layout)
            assert c.stat("fwd_batched", f64, "path_bytes") == want, (geometry, c.where, layout)
    if geometry == "default":
        assert all(int(out[key(*w, "fwd", True, "ranges")]) == gc.SPP for w in gc.cases())


# ---- 2: the plain renders --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", gc.SCENES)
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_plain_renders_f64(pkg, oracle, geometry, name):
    """render (forward-only, backward with an adjoint image, unbiased, loss_l2) and render_gradient_image in the f64 mode against the
    restatement: columns and the role-free f64 kernel (cornell), the glossy lobe, history walked mid-path (cornell_emissive_wall), the
    5 ... 8-parameter forms (random3), the general form (params12), a hiprtc kernel (cornell_disc_box)"""
    out = child(geometry)
    for tracer in range(len(gc.TRACERS)):
        for frame in gc.FRAMES:
            E = expected(pkg, oracle, name, tracer, frame)
            c = Case(out, name, tracer, frame)
            what = (geometry, name, tracer, frame)
            for call in ("fwd", "bwd", "loss_l2", "gimg"):
                plain_counts(c, E, call, True)
                values_f64(geometry, c.get(call, True, "image"), E["image"], what + (call, "image"), floats=True)
            values_f64(geometry, c.get("bwd", True, "grads"), E["grads"], what + ("bwd",))
            values_f64(geometry, c.get("loss_l2", True, "grads"), E["loss_l2"], what + ("loss_l2",))
            values_f64(geometry, c.get("gimg", True, "gimg"), E["gimg"], what + ("gimg",), floats=True)
            uimg, ugrads, usegments = E["unbiased"]
            assert c.stat("unbiased", True, "segments") == usegments, what
            values_f64(geometry, c.get("unbiased", True, "image"), uimg, what + ("unbiased", "image"), floats=True)
            values_f64(geometry, c.get("unbiased", True, "grads"), ugrads, what + ("unbiased",))
            for call in ("fwd", "bwd", "gimg"):
                assert c.stat(call, True, "path_launches") == 1 and c.stat(call, True, "shade_launches") == 0, what + (call,)
            if "disc" in name:
                assert c.stat("bwd", True, "specialised") == 1
    print(f"{geometry} {name}: worst f64 error of the geometry so far {_worst.get(geometry, 0.0):.3e}")


@pytest.mark.parametrize("name", gc.SCENES)
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_plain_renders_f32(pkg, oracle, geometry, name):
    """the same calls in f32: check_f32 of tests/test_gpu_parity.py (flip-aware) for image and gradients, PIXEL_TOL with the flip budget
    for the gradient image"""
    out = child(geometry)
    failures = Failures()
    for tracer in range(len(gc.TRACERS)):
        for frame in gc.FRAMES:
            E = expected(pkg, oracle, name, tracer, frame)
            c = Case(out, name, tracer, frame)
            n_paths = frame[0] * frame[1] * gc.SPP
            heavy = "random" in name
            uimg, ugrads, usegments = E["unbiased"]
            with failures.case(geometry, name, tracer, frame, "fwd"):
                check_f32(c.get("fwd", False, "image"), None, c.stat("fwd", False, "segments"), E["image"], None, E["segments"],
                          heavy_tailed=heavy, n_paths=n_paths)
            for call, image, grads, segments in (("bwd", E["image"], E["grads"], E["segments"]), ("loss_l2", E["image"], E["loss_l2"], E["segments"]),
                                                 ("unbiased", uimg, ugrads, usegments)):
                with failures.case(geometry, name, tracer, frame, call):
                    check_f32(c.get(call, False, "image"), c.get(call, False, "grads"), c.stat(call, False, "segments"), image, grads, segments,
                              heavy_tailed=heavy, n_paths=n_paths)
            with failures.case(geometry, name, tracer, frame, "gimg"):
                pixels_f32(c.get("gimg", False, "gimg"), E["gimg"], n_paths, (geometry, name, tracer, frame, "gimg"))
            assert c.stat("bwd", False, "path_launches") == 1 and c.stat("gimg", False, "path_launches") == 1
    failures.raise_all()


# ---- 3: the derived forms --------------------------------------------------------------------------------------------------------
def derived_f64(geometry, c, E, calls, what):
    x = E["x"]
    target = x.target.astype(np.float64)
    r = E["image"] - target
    for call in calls:
        if call not in ("sets_grad", "cross2"):
            assert c.stat(call, True, "segments") == E["segments"] and c.stat(call, True, "capped_paths") == E["capped"], what + (call,)
        assert c.stat(call, True, "path_launches") == 1 and c.stat(call, True, "shade_launches") == 0, what + (call,)
    if "tangent" in calls:
        values_f64(geometry, c.get("tangent", True, "image"), E["image"], what + ("tangent", "image"))
        values_f64(geometry, c.get("tangent", True, "tangent"), E["T"][0], what + ("tangent",))
    if "tangents" in calls:
        values_f64(geometry, c.get("tangents", True, "image"), E["image"], what + ("tangents", "image"), floats=True)
        for k in range(3):
            values_f64(geometry, c.get("tangents", True, "tangents")[k], E["T"][k], what + ("tangents", k), floats=True)
    if "neq" in calls:
        terms = eq_terms(E["J"], r)
        for f in ("A", "b", "loss"):
            sums_f64(geometry, c.get("neq", True, f), terms[f], what + ("neq", f))
        for p in range(len(E["J"])):
            if np.abs(E["J"][p]).max() > 0:
                values_f64(geometry, c.get("neq", True, "jacobian")[p], E["J"][p], what + ("neq", "jacobian", p), floats=True)
            else:
                assert not c.get("neq", True, "jacobian")[p].any()
        values_f64(geometry, c.get("neq", True, "image"), E["image"], what + ("neq", "image"), floats=True)
    if "along" in calls:
        terms = eq_terms(E["T"], r)
        for f in ("A", "b", "loss"):
            sums_f64(geometry, c.get("along", True, f), terms[f], what + ("along", f))
        for k in range(3):
            values_f64(geometry, c.get("along", True, "tangents")[k], E["T"][k], what + ("along", "tangents", k), floats=True)
    for call, T, image, n in (("cross", E.get("T"), E["image"], gc.SPP), ("cross2", E.get("T2"), E.get("image2"), gc.SPP_CROSS)):
        if call in calls:
            got = {f: c.get(call, True, f) for f in ("A", "b", "loss", "bias", "variance")}
            terms = eq_terms(T, image - target)
            # the sums of absolute terms as tests/test_gpu_cross.py forms them (bounded from below for the corrections): from the restated
            # images and the render's own variance image
            sc = scales({"tangents": T, "image": image, "variance": got["variance"]}, x.target, n)
            b_plain, loss_plain = plain(got)
            for f, value in (("A", got["A"]), ("b", b_plain), ("loss", loss_plain)):
                note(geometry, (np.abs(value - terms[f].sum((0, 1))) / sc[f]).max())
                close(value, terms[f].sum((0, 1)), sc[f], F64_TOL, f"{what} {call} {f}")
            assert np.abs(got["bias"]).max() > 0
            for k in range(3):
                values_f64(geometry, c.get(call, True, "tangents")[k], T[k], what + (call, "tangents", k), floats=True)
            values_f64(geometry, c.get(call, True, "image"), image, what + (call, "image"), floats=True)
    if "sets" in calls:
        for k in range(3):
            values_f64(geometry, c.get("sets", True, "images")[k], E["set_images"][k], what + ("sets", k))
        rk = E["set_images"] - target
        sums_f64(geometry, c.get("sets", True, "loss"), np.moveaxis(rk * rk, 0, 2), what + ("sets", "loss"))
    if "sets_along" in calls:
        rk, tk = E["set_images"][:2] - target, E["set_tangents"]
        for k in range(2):
            values_f64(geometry, c.get("sets_along", True, "images")[k], E["set_images"][k], what + ("sets_along", k))
            values_f64(geometry, c.get("sets_along", True, "tangents")[k], tk[k], what + ("sets_along", "tangent", k))
        for f, terms in (("loss", rk * rk), ("dloss", 2 * rk * tk), ("curv", tk * tk)):
            sums_f64(geometry, c.get("sets_along", True, f), np.moveaxis(terms, 0, 2), what + ("sets_along", f))
    if "sets_grad" in calls:
        assert c.stat("sets_grad", True, "segments") == E["segments"]
        for k in range(3):
            values_f64(geometry, c.get("sets_grad", True, "grads")[k], E["set_grads"][k], what + ("sets_grad", k))


def derived_f32(failures, c, E, calls, what, n_paths):
    target = E["x"].target.astype(np.float64)
    f32 = lambda call, f: np.asarray(c.get(call, False, f), np.float64)

    def equations(call, T_want, image_want, T_got, values):
        aside = np.zeros(image_want.shape[:2], bool)
        for k in range(len(T_want)):
            if np.abs(T_want[k]).max() > 0:
                aside |= pixels_f32(T_got[k], T_want[k], n_paths, what + (call, "image", k))
        aside |= pixels_f32(f32(call, "image"), image_want, n_paths, what + (call, "image"))
        assert aside.sum() <= flip_budget(n_paths)
        got_terms, want_terms = eq_terms(T_got, f32(call, "image") - target), eq_terms(T_want, image_want - target)
        for f in ("A", "b", "loss"):
            sums_f32(values[f], got_terms[f], want_terms[f], aside, what + (call, f))

    def sets(call, n):
        aside = np.zeros(target.shape[:2], bool)
        for k in range(n):
            aside |= pixels_f32(f32(call, "images")[k], E["set_images"][k], n_paths, what + (call, k))
            if call == "sets_along":
                aside |= pixels_f32(f32(call, "tangents")[k], E["set_tangents"][k], n_paths, what + (call, "tangent", k))
        assert aside.sum() <= flip_budget(n_paths)
        rg, rw = f32(call, "images") - target, E["set_images"][:n] - target
        fields = [("loss", rg * rg, rw * rw)]
        if call == "sets_along":
            tg, tw = f32(call, "tangents"), E["set_tangents"]
            fields += [("dloss", 2 * rg * tg, 2 * rw * tw), ("curv", tg * tg, tw * tw)]
        for f, terms_got, terms_want in fields:
            sums_f32(f32(call, f), np.moveaxis(terms_got, 0, 2), np.moveaxis(terms_want, 0, 2), aside, what + (call, f))

    for call in calls:
        with failures.case(*what, call):
            assert c.stat(call, False, "path_launches") == 1 and c.stat(call, False, "shade_launches") == 0
            if call != "cross2":
                assert abs(c.stat(call, False, "segments") - E["segments"]) <= 64
            if call == "tangent":
                pixels_f32(f32("tangent", "tangent"), E["T"][0], n_paths, what + ("tangent",))
                pixels_f32(f32("tangent", "image"), E["image"], n_paths, what + ("tangent", "image"))
            elif call == "tangents":
                for k in range(3):
                    pixels_f32(f32("tangents", "tangents")[k], E["T"][k], n_paths, what + ("tangents", k))
            elif call == "neq":
                equations("neq", E["J"], E["image"], f32("neq", "jacobian"), {f: f32("neq", f) for f in ("A", "b", "loss")})
            elif call == "along":
                equations("along", E["T"], E["image"], f32("along", "tangents"), {f: f32("along", f) for f in ("A", "b", "loss")})
            elif call in ("cross", "cross2"):
                b_plain, loss_plain = plain({f: f32(call, f) for f in ("b", "loss", "bias")})
                equations(call, E["T" if call == "cross" else "T2"], E["image" if call == "cross" else "image2"], f32(call, "tangents"),
                          {"A": f32(call, "A"), "b": b_plain, "loss": loss_plain})
            elif call in ("sets", "sets_along"):
                sets(call, 3 if call == "sets" else 2)
            elif call == "sets_grad":
                for k in range(3):
                    err = np.abs(f32("sets_grad", "grads")[k] - E["set_grads"][k]).max() / np.abs(E["set_grads"][k]).max()
                    assert err <= GRAD_TOL, what + ("sets_grad", k, err)


DERIVED_SCENES = gc.DERIVED + tuple(gc.DERIVED_SOME)


@pytest.mark.parametrize("name", DERIVED_SCENES)
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_derived_forms_f64(pkg, oracle, geometry, name):
    """render_tangent, render_tangents (3 directions), render_normal_equations with its Jacobian images (cornell), _along, _cross (at 7 and
    at 2 samples), render_param_sets (3 sets and a target), _along (2 sets), _grad (3 sets, an adjoint each) in the f64 mode against the
    restatement; the cross form's A, b + bias and loss + bias[K] against the restated plain values"""
    out = child(geometry)
    for tracer in range(len(gc.TRACERS)):
        for frame in gc.FRAMES:
            derived_f64(geometry, Case(out, name, tracer, frame), expected(pkg, oracle, name, tracer, frame), gc.derived_calls(name),
                        (geometry, name, tracer, frame))
    print(f"{geometry} {name}: worst f64 error of the geometry so far {_worst.get(geometry, 0.0):.3e}")


@pytest.mark.parametrize("name", DERIVED_SCENES)
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_derived_forms_f32(pkg, oracle, geometry, name):
    """the same calls in f32: PIXEL_TOL with the flip budget for every image, GRAD_TOL of the sum of absolute terms for every sum, GRAD_TOL
    of the largest component for the sets' gradients"""
    out = child(geometry)
    failures = Failures()
    for tracer in range(len(gc.TRACERS)):
        for frame in gc.FRAMES:
            derived_f32(failures, Case(out, name, tracer, frame), expected(pkg, oracle, name, tracer, frame), gc.derived_calls(name),
                        (geometry, name, tracer, frame), frame[0] * frame[1] * gc.SPP)
    failures.raise_all()


# ---- 4: batches, and geometry against geometry -----------------------------------------------------------------------------------
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_batched_renders_equal_the_unbatched(geometry):
    """9 x 5 in batches of 4 paths (one pixel per batch, its samples cut 4 + 3) and 23 x 11 in batches of 253 * 3 + 5 (pixels cut
    mid-group) against the SAME child's unbatched render: equal segments and capped paths; f64 within F64_TOL of the largest component
    (+ 2^-24 for the float image), f32 -- the same paths in the same arithmetic, other sums -- within PIXEL_TOL and GRAD_TOL, no pixel set
    aside"""
    out = child(geometry)
    for name, tracer, frame in gc.cases():
        c = Case(out, name, tracer, frame)
        for f64 in (True, False):
            for call in ("fwd", "bwd"):
                assert c.stat(call + "_batched", f64, "batches") > 1
                for s in ("segments", "capped_paths"):
                    assert c.stat(call + "_batched", f64, s) == c.stat(call, f64, s), (geometry, c.where, call, s)
                one, many = c.get(call, f64, "image").astype(np.float64), c.get(call + "_batched", f64, "image").astype(np.float64)
                assert np.abs(many - one).max() <= ((F64_TOL + F32_EPS) if f64 else PIXEL_TOL) * np.abs(one).max(), (geometry, c.where, call)
            one, many = c.get("bwd", f64, "grads"), c.get("bwd_batched", f64, "grads")
            assert np.abs(many - one).max() <= (F64_TOL if f64 else GRAD_TOL) * np.abs(one).max(), (geometry, c.where, "grads")


SUMS = ("A", "b", "loss", "bias", "dloss", "curv")


@pytest.mark.parametrize("geometry", OTHERS)
def test_f64_against_the_default_geometry(pkg, oracle, geometry):
    """every f64 output of the geometry against the `default` child's (ranges of one sample): equal statistics; 1e-9 of the largest
    component (+ 2^-24 for float images), 1e-9 of the sum of absolute terms for reduced sums -- the cross form's `bias` and variance image
    have no other reference.  Which outputs agree bit for bit is printed per call, not asserted; the f32 corrections of the cross form within
    GRAD_TOL of the sum of absolute terms"""
    out, base = child(geometry), child("default")
    same, differ = {}, {}
    for k in sorted(base):
        parts = k.split("/")
        if len(parts) != 6:
            continue
        name, tracer, frame, call, prec, field = parts
        if prec != "f64" or field == "ranges":
            continue
        a, b = out[k], base[k]
        if field == "stats":
            for s in ("segments", "capped_paths", "batches", "path_launches", "shade_launches", "specialised"):
                assert a[gc.STATS.index(s)] == b[gc.STATS.index(s)], (geometry, k, s)
            continue
        (same if np.array_equal(a, b) else differ).setdefault(call, []).append(k)
        if field in SUMS and call in ("cross", "cross2"):
            w, h = (int(v) for v in frame.split("x"))
            x = gc.inputs(pkg, name, int(tracer), (w, h))
            n = gc.SPP if call == "cross" else gc.SPP_CROSS
            got = {f: base[k[:-len(field)] + f] for f in ("tangents", "image", "variance")}
            close(a, b, scales(got, x.target, n)[field], F64_TOL, f"{geometry} {k}")
            a32, b32 = out[k.replace("/f64/", "/f32/")], base[k.replace("/f64/", "/f32/")]
            close(a32, b32, scales(got, x.target, n)[field], GRAD_TOL, f"{geometry} {k} f32")
        elif field in SUMS:
            w, h = (int(v) for v in frame.split("x"))
            terms = restated_terms(expected(pkg, oracle, name, int(tracer), (w, h)), call)[field]
            close(a, b, np.abs(terms).sum((0, 1)), F64_TOL, f"{geometry} {k}")
        else:
            floats = a.dtype == np.float32
            err = np.abs(a.astype(np.float64) - b.astype(np.float64)).max() / max(np.abs(b).max(), 1e-300)
            assert err <= F64_TOL + (F32_EPS if floats else 0.0), (geometry, k, err)
    for call in sorted(set(same) | set(differ)):
        n_same, n_differ = len(same.get(call, [])), len(differ.get(call, []))
        print(f"{geometry} against default, {call}: {n_same} outputs bit-identical, {n_differ} not" +
              (f" (first: {differ[call][0]})" if n_differ else ""))
    print(f"{geometry}: worst f64 error against the restatement {_worst.get(geometry, float('nan')):.3e}, "
          f"child {float(out['seconds']):.1f} s")
