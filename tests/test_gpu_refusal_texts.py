"""Every refusal of the six families of entry points that run on the one-launch path kernel's special forms -- drt_hip_render_tangent /
_double, _render_normal_equations, _render_tangents, _render_normal_equations_along, _render_param_sets / _double, _render_param_sets_along /
_double -- with its status and its COMPLETE message, compared with ==.  The other GPU files match a word or two of each message; this one pins the bytes, so that the
checks the families share can live in one place without a caller seeing a difference.

All calls go straight through the C ABI (the Python mirror refuses some shapes and values before the call).  The frame is the 16 x 12
Cornell box at 2 spp, depth 3.  No refusal below traces a path: the rows refused only once the shard is planned (paths that end at depth 0)
and drt_hip_render_tangent's bad camera, which the plain render's checks refuse, come after the staging launch and the memsets, nothing more.
Conditions that need a forced DRT_HIP_* setting are not here.

The scene above the parameter cap is many_param_scene(126), the largest that function builds, with eleven spare parameters: 137 in all."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 16, 12
ARGS = {
    "render_tangent": ("dirs", "rgb", "timg"),
    "render_tangent_double": ("dirs", "rgb64", "timg64"),
    "render_normal_equations": ("target", "residual", "rgb", "A", "b", "loss", "jac"),
    "render_tangents": ("n", "dirs", "rgb", "jac"),
    "render_normal_equations_along": ("n", "dirs", "target", "residual", "rgb", "A", "b", "loss", "jac"),
    "render_param_sets": ("n", "dirs", "target", "jac", "loss", "rgb"),
    "render_param_sets_double": ("n", "dirs", "target", "jac64", "loss", "rgb"),
    "render_param_sets_along": ("n", "dirs", "dirs2", "target", "jac", "timgs", "loss", "dloss", "curv"),
    "render_param_sets_along_double": ("n", "dirs", "dirs2", "target", "jac64", "timgs64", "loss", "dloss", "curv"),
}
# what a call passes unless its row says otherwise (a valid call of each entry point); "dirs" are the directions / the sets, "dirs2" the
# directions of the sets
DEFAULTS = {"n": 2, "residual": None, "rgb": None}
NE, ALONG, TS, PS, PSD, RT, RTD = ("render_normal_equations", "render_normal_equations_along", "render_tangents", "render_param_sets",
                                  "render_param_sets_double", "render_tangent", "render_tangent_double")
PSA, PSAD = "render_param_sets_along", "render_param_sets_along_double"
FLAGS = ("RENDER_UNFUSED", "RENDER_UNBIASED", "RENDER_LOSS_L2", "RENDER_ALLREDUCE", "RENDER_ALLREDUCE_ASYNC")
TOO_MANY_SAMPLES = (1 << 31) // (W * H) + 1          # W x H x spp just above 2^31 - 1

INFLIGHT = "asynchronous frames are in flight -- drt_hip_wait for them first"
MESH = "not of a scene that holds a triangle mesh"
BPL = "they come from the one-launch path kernel -- not with bounces_per_launch >= 1"
SAMPLES = "more than 2^31 camera samples in one frame (the shard renders in one batch)"
CAP136 = "more parameters than the path kernels stage (136)"
RT_NULL = "render_tangent: NULL render parameters, tangent or output"
RT_FLAGS = "render_tangent: forward mode takes no reverse-mode flag (DRT_RENDER_BACKWARD, _UNBIASED, _LOSS_L2, _ALLREDUCE*)"
RT_BPL = ("render_tangent: the tangent image comes from the one-launch path kernel -- not with bounces_per_launch >= 1 "
          "or DRT_RENDER_UNFUSED")
NE_FLAGS = ("normal equations: not with DRT_RENDER_UNFUSED, _UNBIASED, _LOSS_L2 or _ALLREDUCE* -- the biased operator on the "
            "one-launch path kernel, one context")
FWD_FLAGS = "not with DRT_RENDER_UNFUSED, _UNBIASED, _LOSS_L2 or _ALLREDUCE* -- forward mode on the one-launch path kernel, one context"
SETS_FLAGS = "not with DRT_RENDER_UNFUSED, _UNBIASED, _LOSS_L2 or _ALLREDUCE* -- a forward render on the one-launch path kernel, one context"
NE_CAP_USER = ("normal equations: more than DRT_FAST_PARAMS = 8 parameters (the Jacobian is the path kernel's gradient "
               "columns, which stop there; J^T J v by drt_hip_render_tangent + drt_hip_render is the matrix-free route)")
NE_CAP_MIRROR = ("normal equations: the scene's parameters and the constant a mirror material adds take more than DRT_FAST_PARAMS = 8 "
                 "gradient columns of the path kernel (a mirror costs one: at most 7 parameters beside it)")
BAD_CAMERA = "bad camera or render parameters"

# (where, entry point, how to provoke, status, complete message).  `where`: the context and scene the row runs on.  `how`: arguments
# replaced ("cam": a camera, or None for NULL; "rp": a dict of RenderParams fields, or None for NULL; "flags": or-ed into rp.flags;
# "bad": a value stored into "dirs"; "bad2": into "dirs2", at the same index; "bad_target": a value stored into the target)
ROWS = []


def row(where, fn, how, status, message):
    ROWS.append((where, fn, how, status, message))


# ---- what the K-direction forms, the parameter sets and the Jacobian form share, each in its own words
for fn, who, group_hint in ((NE, "normal equations", " (render the shards on plain contexts and add them)"),
                            (TS, "tangents", " (render the shards on plain contexts)"),
                            (ALONG, "normal equations along", " (render the shards on plain contexts)"),
                            (PS, "param sets", " (render the shards on plain contexts)"),
                            (PSD, "param sets", " (render the shards on plain contexts)"),
                            (PSA, "param sets along", " (render the shards on plain contexts)"),
                            (PSAD, "param sets along", " (render the shards on plain contexts)")):
    row("group", fn, {}, "DRT_ERR_UNSUPPORTED", f"{who}: not on a group context{group_hint}")
    row("empty", fn, {}, "DRT_ERR_NO_SCENE", "render before upload_scene")
    for how in ({"cam": None}, {"rp": None}, {"cam": (0, H)}, {"cam": (W, -1)}):
        row("cornell", fn, how, "DRT_ERR_INVALID", f"{who}: {BAD_CAMERA}")
    row("inflight", fn, {}, "DRT_ERR_INVALID", f"{who}: {INFLIGHT}")
    for flag in FLAGS:
        row("cornell", fn, {"flags": flag}, "DRT_ERR_UNSUPPORTED", NE_FLAGS if fn == NE else f"{who}: {SETS_FLAGS if fn in (PS, PSD, PSA, PSAD) else FWD_FLAGS}")
    row("mesh", fn, {}, "DRT_ERR_UNSUPPORTED", f"{who}: {MESH}")
    row("cornell", fn, {"rp": {"bounces_per_launch": 1}}, "DRT_ERR_UNSUPPORTED", f"{who}: {BPL}")
    row("many137", fn, {}, "DRT_ERR_UNSUPPORTED", NE_CAP_USER if fn == NE else f"{who}: {CAP136}")
    row("cornell", fn, {"rp": {"spp": TOO_MANY_SAMPLES}, "target": None, "loss": None} if fn in (PS, PSD)
        else {"rp": {"spp": TOO_MANY_SAMPLES}, "target": None, "loss": None, "dloss": None} if fn in (PSA, PSAD) else {"rp": {"spp": TOO_MANY_SAMPLES}},
        "DRT_ERR_UNSUPPORTED", f"{who}: {SAMPLES}")

# ---- paths that end at depth 0 never reach the path kernel: refused once the shard is planned, in the form's words
DEPTH0 = {"rp": {"min_bounces": 0}}
IN_ONE_BATCH = ("batch, which this render does not take (a DRT_HIP_* setting that forces the queue wavefront or a batch size, "
                "more than 2^31 camera samples, or a scene its intersection program does not cover)")
row("cornell", NE, DEPTH0, "DRT_ERR_UNSUPPORTED",
    "normal equations: they come from the one-launch path kernel's Jacobian form over the whole shard in one " + IN_ONE_BATCH)
for fn in (TS, ALONG):
    row("cornell", fn, DEPTH0, "DRT_ERR_UNSUPPORTED",
        "tangents / normal equations along: they come from the one-launch path kernel's K-direction form over the whole shard in one " + IN_ONE_BATCH)
for fn in (PS, PSD):
    row("cornell", fn, DEPTH0, "DRT_ERR_UNSUPPORTED",
        "param sets: they come from the one-launch path kernel's parameter-set form over the whole shard in one batch, "
        "which this render does not take (a DRT_HIP_* setting that forces the queue wavefront or a batch size, paths "
        "that end at depth 0, or a scene its intersection program does not cover)")
for fn in (PSA, PSAD):
    row("cornell", fn, DEPTH0, "DRT_ERR_UNSUPPORTED",
        "param sets along: they come from the one-launch path kernel's parameter-set form with directions over the whole shard in one batch, "
        "which this render does not take (a DRT_HIP_* setting that forces the queue wavefront or a batch size, paths "
        "that end at depth 0, or a scene its intersection program does not cover)")

# ---- the Jacobian form's own
row("mirror8", NE, {}, "DRT_ERR_UNSUPPORTED", NE_CAP_MIRROR)
row("cornell", NE, {"residual": "target"}, "DRT_ERR_INVALID", "normal equations: exactly one of target_rgb and residual_rgb")
row("cornell", NE, {"target": None}, "DRT_ERR_INVALID", "normal equations: exactly one of target_rgb and residual_rgb")
row("cornell", NE, {"A": None}, "DRT_ERR_INVALID", "normal equations: NULL out_A or out_b")
row("cornell", NE, {"b": None}, "DRT_ERR_INVALID", "normal equations: NULL out_A or out_b")
for bad in (np.nan, np.inf):
    row("cornell", NE, {"bad_target": bad}, "DRT_ERR_INVALID", "normal equations: the target / residual image holds a value that is not finite")
    row("cornell", ALONG, {"bad_target": bad}, "DRT_ERR_INVALID", "normal equations along: the target / residual image holds a value that is not finite")

# ---- the K-direction forms' own
for fn, who in ((TS, "tangents"), (ALONG, "normal equations along")):
    for n in (0, 9, -1):
        row("cornell", fn, {"n": n}, "DRT_ERR_INVALID", f"{who}: n_dirs outside 1 ... DRT_HIP_MAX_DIRS = 8")
    row("cornell", fn, {"dirs": None}, "DRT_ERR_INVALID", f"{who}: NULL directions or output")
    for bad in (np.nan, np.inf):
        row("cornell", fn, {"bad": bad}, "DRT_ERR_INVALID", f"{who}: a direction holds a value that is not finite")
row("cornell", TS, {"jac": None}, "DRT_ERR_INVALID", "tangents: NULL directions or output")
row("cornell", ALONG, {"A": None}, "DRT_ERR_INVALID", "normal equations along: NULL directions or output")
row("cornell", ALONG, {"b": None}, "DRT_ERR_INVALID", "normal equations along: NULL directions or output")
row("cornell", ALONG, {"residual": "target"}, "DRT_ERR_INVALID", "normal equations along: exactly one of target_rgb and residual_rgb")
row("cornell", ALONG, {"target": None}, "DRT_ERR_INVALID", "normal equations along: exactly one of target_rgb and residual_rgb")

# ---- the parameter sets' own
for fn in (PS, PSD):
    for n in (0, 9, -1):
        row("cornell", fn, {"n": n}, "DRT_ERR_INVALID", "param sets: n_sets outside 1 ... DRT_HIP_MAX_PARAM_SETS = 8")
    row("cornell", fn, {"dirs": None}, "DRT_ERR_INVALID", "param sets: NULL param_sets")
    row("cornell", fn, {"jac": None, "jac64": None, "loss": None}, "DRT_ERR_INVALID", "param sets: no output requested (out_images and out_loss are both NULL)")
    row("cornell", fn, {"target": None}, "DRT_ERR_INVALID", "param sets: out_loss needs target_rgb")
    row("cornell", fn, {"flags": "RENDER_BACKWARD"}, "DRT_ERR_INVALID", "param sets: a forward render: no DRT_RENDER_BACKWARD")
    for bad in (np.nan, np.inf):
        row("cornell", fn, {"bad": bad}, "DRT_ERR_INVALID", "param sets: a set holds a value that is not finite")
        row("cornell", fn, {"bad_target": bad}, "DRT_ERR_INVALID", "param sets: the target image holds a value that is not finite")
    row("cornell", fn, {"n": 8, "rgb": "rgb"}, "DRT_ERR_UNSUPPORTED",
        "param sets: out_rgb beside 8 sets (the plain image takes one of the kernel's eight: drt_hip_render gives it)")
row("cornell", PSD, {"flags": "RENDER_DEVICE_OUT"}, "DRT_ERR_INVALID",
    "param sets: the double images come through host buffers only (no DRT_RENDER_DEVICE_OUT)")

# ---- the parameter sets with a direction each: their own
for fn in (PSA, PSAD):
    for n in (0, 5, -1):
        row("cornell", fn, {"n": n}, "DRT_ERR_INVALID", "param sets along: n_sets outside 1 ... DRT_HIP_MAX_SETS_ALONG = 4")
    for array in ("dirs", "dirs2"):
        row("cornell", fn, {array: None}, "DRT_ERR_INVALID", "param sets along: NULL param_sets or param_tangents")
    row("cornell", fn, {"jac": None, "jac64": None, "timgs": None, "timgs64": None, "loss": None, "dloss": None, "curv": None}, "DRT_ERR_INVALID",
        "param sets along: no output requested (out_images, out_tangents, out_loss, out_dloss and out_curv are all NULL)")
    for other in ("dloss", "loss"):                      # out_loss alone, out_dloss alone
        row("cornell", fn, {"target": None, other: None}, "DRT_ERR_INVALID", "param sets along: out_loss and out_dloss need target_rgb")
    row("cornell", fn, {"flags": "RENDER_BACKWARD"}, "DRT_ERR_INVALID", "param sets along: a forward render: no DRT_RENDER_BACKWARD")
    for bad in (np.nan, np.inf):
        row("cornell", fn, {"bad": bad}, "DRT_ERR_INVALID", "param sets along: a set holds a value that is not finite")
        row("cornell", fn, {"bad2": bad}, "DRT_ERR_INVALID", "param sets along: a direction holds a value that is not finite")
        row("cornell", fn, {"bad_target": bad}, "DRT_ERR_INVALID", "param sets along: the target image holds a value that is not finite")
    # (both arrays bad at the same index: the set is looked at first)
    row("cornell", fn, {"bad": np.nan, "bad2": np.inf}, "DRT_ERR_INVALID", "param sets along: a set holds a value that is not finite")
row("cornell", PSAD, {"flags": "RENDER_DEVICE_OUT"}, "DRT_ERR_INVALID",
    "param sets along: the double images come through host buffers only (no DRT_RENDER_DEVICE_OUT)")

# ---- forward mode along one direction: the oldest form, in its own words throughout
for fn in (RT, RTD):
    row("group", fn, {}, "DRT_ERR_UNSUPPORTED", "render_tangent: not on a group context")
    row("empty", fn, {}, "DRT_ERR_NO_SCENE", "render before upload_scene")
    for how in ({"rp": None}, {"dirs": None}, {"timg": None, "timg64": None}):
        row("cornell", fn, how, "DRT_ERR_INVALID", RT_NULL)
    for flag in ("RENDER_BACKWARD",) + FLAGS[1:]:
        row("cornell", fn, {"flags": flag}, "DRT_ERR_INVALID", RT_FLAGS)
    for bad in (np.nan, np.inf):
        row("cornell", fn, {"bad": bad}, "DRT_ERR_INVALID", "render_tangent: the tangent holds a value that is not finite")
    row("inflight", fn, {}, "DRT_ERR_INVALID", f"render: {INFLIGHT}")
    row("mesh", fn, {}, "DRT_ERR_UNSUPPORTED", "render_tangent: no tangent image of a scene that holds a triangle mesh")
    row("cornell", fn, {"rp": {"bounces_per_launch": 1}}, "DRT_ERR_UNSUPPORTED", RT_BPL)
    row("cornell", fn, {"flags": "RENDER_UNFUSED"}, "DRT_ERR_UNSUPPORTED", RT_BPL)
    row("many137", fn, {}, "DRT_ERR_UNSUPPORTED", "render_tangent: a tangent of more parameters than the path kernels stage (136)")
    for how in ({"cam": None}, {"cam": (0, H)}, {"cam": (W, -1)}):
        row("cornell", fn, how, "DRT_ERR_INVALID", f"render: {BAD_CAMERA}")
row("cornell", RTD, {"flags": "RENDER_DEVICE_OUT"}, "DRT_ERR_INVALID", "render_tangent_double: host buffers only")

WHERE = ("cornell", "inflight", "mesh", "many137", "mirror8", "empty", "group")
assert {r[0] for r in ROWS} == set(WHERE)


def scene_for(pkg, where):
    if where == "mesh":
        return pkg.scene_by_name("mesh6x8")
    if where in ("many137", "mirror8"):
        s = pkg.many_param_scene(126) if where == "many137" else pkg.cornell_box(front_mirror=True)
        while s.n_params < (137 if where == "many137" else 8):
            s.parameter((0.5, 0.5, 0.5), True, f"spare{s.n_params}")
        return s
    return pkg.cornell_box()


def provoke(pkg, r, fn, how):
    """one call of `fn` with valid arguments except for `how` -> (status name, message)"""
    P = r.scene.n_params if r.scene is not None else 4
    a = dict(DEFAULTS)
    a["dirs"] = np.random.RandomState(5).uniform(0.1, 0.9, (9, P, 3))
    a["dirs2"] = np.random.RandomState(7).uniform(-1, 1, (9, P, 3))
    a["target"] = np.random.RandomState(6).uniform(0, 1, (H, W, 3)).astype(np.float32)
    if "bad" in how:
        a["dirs"][1 if fn not in (RT, RTD) else 0, 2, 1] = how["bad"]
    if "bad2" in how:
        a["dirs2"][1, 2, 1] = how["bad2"]
    if "bad_target" in how:
        a["target"][3, 5, 1] = how["bad_target"]
    n_rows = max(P, 9)
    for name, shape, dtype in (("timg", (H, W, 3), np.float32), ("timg64", (H, W, 3), np.float64), ("rgb64", (H, W, 3), np.float64),
                               ("A", (3, n_rows, n_rows), np.float64), ("b", (3, n_rows), np.float64), ("loss", (n_rows, 3), np.float64),
                               ("dloss", (n_rows, 3), np.float64), ("curv", (n_rows, 3), np.float64),
                               ("timgs", (n_rows, H, W, 3), np.float32), ("timgs64", (n_rows, H, W, 3), np.float64),
                               ("jac", (n_rows, H, W, 3), np.float32), ("jac64", (n_rows, H, W, 3), np.float64)):
        a[name] = np.zeros(shape, dtype)
    spare_rgb = np.zeros((H, W, 3), np.float32)
    for k, v in how.items():
        if k in ARGS[fn] or k in a:
            a[k] = {"target": a["target"], "rgb": spare_rgb}[v] if isinstance(v, str) else v
    rp = pkg.RenderParams(spp=2, seed=3, min_bounces=3, absorb=1.0)
    d = cd = None
    if how.get("rp", {}) is not None:
        rp = dataclasses.replace(rp, **how.get("rp", {}))
        d = rp.to_desc()
        d.flags = rp.flags | (getattr(pkg, how["flags"]) if "flags" in how else 0)
    if how.get("cam", ()) is not None:
        cd = pkg.cornell_camera(*how.get("cam", (W, H))).to_desc()

    def c(v):
        return v if isinstance(v, int) else (v.ctypes.data_as(C.c_void_p) if v is not None else None)
    rc = getattr(r.lib, "drt_hip_" + fn)(r.ctx, C.byref(cd) if cd is not None else None, C.byref(d) if d is not None else None,
                                         *[c(a[k]) for k in ARGS[fn]], None)
    msg = r.lib.drt_hip_last_error(r.ctx)
    return pkg.STATUS_NAMES.get(rc, rc), msg.decode() if msg else ""


@pytest.mark.parametrize("where", WHERE)
def test_every_refusal_keeps_its_status_and_its_text(pkg, hip, where):
    cam = pkg.cornell_camera(W, H)
    rp = pkg.RenderParams(spp=2, seed=3, min_bounces=3, absorb=1.0)
    r = pkg.HipRenderer([0, 0]) if where == "group" else pkg.HipRenderer(0) if where == "empty" else hip
    handle = None
    try:
        if where != "empty":
            r.upload_scene(scene_for(pkg, where))
        if where == "inflight":
            handle = r.render_async(cam, rp)
        got = [(fn, how, *provoke(pkg, r, fn, how)) for w, fn, how, _, _ in ROWS if w == where]
    finally:
        if handle is not None:
            r.wait(handle)
        if r is not hip:
            r.close()
    want = [(fn, how, status, message) for w, fn, how, status, message in ROWS if w == where]
    wrong = [(g, w[2:]) for g, w in zip(got, want) if g[2:] != w[2:]]
    assert not wrong, "\n".join(f"{g[0]} {g[1]}: got {g[2:]}, expected {w}" for g, w in wrong)
    if where not in ("empty", "group"):          # the context is what it was: it renders
        assert hip.render(cam, rp)[0].max() > 0
