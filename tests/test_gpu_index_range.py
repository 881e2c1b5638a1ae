"""Frames whose camera-sample indices reach the top of the 32-bit range: every route of the library on single rows of a 2^32-sample frame.

A camera sample's index pixel * spp + sample is its path's RNG key.  drt_hip_render accepts a frame of up to exactly 2^32 samples; the
largest index any other test renders is about 2^28.  Up there live the sign bit (an int conversion, a signed compare, a sign-extending
widening), the float bit patterns of the adjoint-round wavefront's packed key (+Inf, signalling and quiet NaNs, -0, negative denormals,
negative NaNs: tests/index_range.py, PATTERNS), the launch geometry of a pixel of 4096 samples (4096 sample ranges of one sample for one
pixel group) and the refusal at 2^32 itself.  A render of one image row (band_rows = 1, n_shards = H, shard = row) traces 120,040 to
262,144 paths with the FRAME's pixel numbers, so all of it is cheap to reach.

Expected values are the fp64 restatement's (oracle.render with the same shard fields, a 64-bit path index), computed once per (family,
row) in tests/index_range.py and shared.  Bounds are the project's stated ones, none new:
  * f64: gradients 1e-9 of the largest component, equal segments, capped_paths == 0, the shard's row rtol 2e-7 (test_edge_cases), the rows
    the shard does not own untouched (the caller's buffer keeps what it held).
  * f32: check_f32 of tests/test_gpu_parity.py with flip_budget for the paths of the row; on the mesh check_f32_heavy_tailed with the
    restatement's gradient images.  The seeds are the first at which the restatement alone calls the row stable (tests/index_range.py,
    SEEDS; re-derived by tests/test_index_range_inputs.py).  The families no seed makes stable (F64_ONLY: the 12-parameter room and the
    glossy sphere at thousands of samples a pixel) keep the f64 pin and, in f32, the route-against-route terms of
    tests/test_gpu_many_params.py and test_results_do_not_depend_on_bounces_per_launch.
  * unbiased f32: route against route, and 1e-5 against the restatement (test_unbiased_backward_matches_reference) on the stable rows.

pytest -s prints every figure (profiles/r23_index_range.txt is the first run's)."""
import dataclasses
import time

import numpy as np
import pytest

import f32_flips as ff
import index_range as ir
from test_gpu_parity import GRAD_TOL_HEAVY, PIXEL_TOL, check_f32, check_f32_heavy_tailed, flip_budget, grad_rel_err

pytestmark = pytest.mark.gpu

F64_TOL = 1e-9
UNBIASED_F32 = 1e-5                      # test_unbiased_backward_matches_reference
SENTINEL = np.float32(-7.0)              # what the caller's image buffer holds before a render
GIMG_PARAM = 2                           # a BxDF's colour in both scenes (cornell's white, params12's albedo2): tests/geometry_child.py
rows = pytest.mark.parametrize("where", ir.RENDER_ROWS, ids=[f"{f}-{r}" for f, r in ir.RENDER_ROWS])


def say(where, what, **figures):
    print(f"index_range {where[0]}-{where[1]} {what}: " + ", ".join(f"{k} {v:.3e}" if isinstance(v, float) else f"{k} {v}" for k, v in figures.items()))


def render(hip, x, rp=None, owned=None, **kw):
    """hip.render into a buffer that holds SENTINEL: the rows the shard does not own must still hold it afterwards"""
    img = np.full((x.cam.height, x.cam.width, 3), SENTINEL, np.float32)
    out = hip.render(x.cam, rp or x.rp, img_out=img, **kw)
    mine = np.zeros(x.cam.height, bool)
    mine[[x.where[1]] if owned is None else list(owned)] = True
    assert (img[~mine] == SENTINEL).all(), "a row the shard does not own was written"
    assert np.isfinite(img[mine]).all()
    return out


def pin_f64(x, what, got, ref, owned=None):
    """the f64 mode against the restatement -> the gradient error"""
    img, grads, st = got
    own = [x.where[1]] if owned is None else list(owned)
    assert st["segments"] == ref["stats"]["segments"] and st["capped_paths"] == 0, (what, st["segments"], ref["stats"]["segments"])
    assert st["paths"] == ref["stats"]["paths"] == len(own) * ir.row_paths(x.where)
    np.testing.assert_allclose(img[own], ref["image"][own].astype(np.float32), rtol=2e-7, atol=1e-12)
    err = 0.0
    if grads is not None:
        err = grad_rel_err(grads, ref["grads"])
        assert err < F64_TOL, (what, err)
    say(x.where, what + " f64", segments=st["segments"], grad_err=err)
    return err


def strict_f32(x, what, got, ref):
    """check_f32 on the shard's row, the flip budget that of the row's paths"""
    img, grads, st = got
    row = x.where[1]
    bad = int((np.abs(img[row].astype(np.float64) - ref["image"][row]).max(-1) > PIXEL_TOL * np.abs(ref["image"][row]).max()).sum())
    say(x.where, what + " f32", flipped_pixels=bad, segment_diff=int(st["segments"]) - ref["stats"]["segments"],
        grad_err=grad_rel_err(grads, ref["grads"]) if grads is not None else 0.0)
    check_f32(img[row][None], grads, st["segments"], ref["image"][row][None], ref["grads"] if grads is not None else None,
              ref["stats"]["segments"], n_paths=ir.row_paths(x.where))


def heavy_f32(hip, oracle, x, what, ref):
    """check_f32_heavy_tailed with the restatement's gradient images, the cap the flip budget of the row's paths"""
    rec = check_f32_heavy_tailed(hip, x.cam, x.rp, None, x.scene.n_params, ref["image"], ref["grads"], ref["stats"]["segments"],
                                 lambda p: ir.expected(oracle, x, ("gimg", p))["grad_image"], max_bad=flip_budget(ir.row_paths(x.where)),
                                 grad_tol=GRAD_TOL_HEAVY, params=ff.wanted(x.scene))
    print(f"index_range {x.where[0]}-{x.where[1]} {what} ", end="")
    ff.report(what, rec)


def routes_f32(x, what, one, queue, unbiased=False):
    """f32, the one-launch route against the queue route.  The general form runs the same arithmetic per vertex on both
    (tests/test_gpu_many_params.py: equal segments, 2e-5 of the largest component); k_path_unbiased and the lean kernels have a closest-hit
    arithmetic of their own (test_results_do_not_depend_on_bounces_per_launch: a flipped path's length -- depth^2 / 2 under the unbiased
    operator, depth <= 64 -- and rtol 2e-5, atol 1e-6 of the largest component)"""
    (_, g1, s1), (_, gq, sq) = one, queue
    say(x.where, what + " f32 routes", segment_diff=int(s1["segments"]) - int(sq["segments"]), grad_diff=grad_rel_err(g1, gq))
    if x.family == "general":
        assert s1["segments"] == sq["segments"] and grad_rel_err(g1, gq) <= 2e-5
    else:
        assert abs(int(s1["segments"]) - int(sq["segments"])) <= (64 * 64 // 2 if unbiased else 64)
        np.testing.assert_allclose(g1, gq, rtol=2e-5, atol=1e-6 * np.abs(gq).max())


@pytest.fixture
def timed(request):
    t0 = time.time()
    yield
    print(f"index_range wall {request.node.name}: {time.time() - t0:.2f} s")


# ---- 1: fixed depth 4 -------------------------------------------------------------------------------------------------------------
@rows
def test_fixed_depth(pkg, hip, oracle, where, timed):
    """cornell, min_bounces = 4, absorb = 1: forward only, backward, backward with an adjoint image.  f32: k_path_lean and the role-
    specialised kernels; f64: the literal k_path."""
    x = ir.inputs(pkg, "depth4", where)
    hip.upload_scene(x.scene)
    bwd, adj = ir.expected(oracle, x, "bwd"), ir.expected(oracle, x, "adj")
    for f64, check in ((True, pin_f64), (False, strict_f32)):
        check(x, "depth4 fwd", render(hip, x, f64=f64), bwd)
        got = render(hip, x, backward=True, f64=f64)
        assert got[2]["kernels"]["path"]["launches"] == 1 and got[2]["kernels"]["shade"]["launches"] == 0
        check(x, "depth4 bwd", got, bwd)
        check(x, "depth4 adj", render(hip, x, backward=True, adjoint=ir.adjoint_of(x), f64=f64), adj)


# ---- 2: the regenerating form -----------------------------------------------------------------------------------------------------
@rows
def test_regenerating_form(pkg, hip, oracle, where, timed):
    """cornell, min_bounces = 1, absorb = 0.5, backward"""
    x = ir.inputs(pkg, "regen", where)
    hip.upload_scene(x.scene)
    ref = ir.expected(oracle, x, "bwd")
    for f64, check in ((True, pin_f64), (False, strict_f32)):
        got = render(hip, x, backward=True, f64=f64)
        assert got[2]["kernels"]["path"]["launches"] == 1
        check(x, "regen bwd", got, ref)


# ---- 3: the general form, and gradient images -------------------------------------------------------------------------------------
@rows
def test_general_form(pkg, hip, oracle, where, timed):
    """params12, min_bounces = 3, absorb = 0.3, backward: history words and per-wave tables.  No seed makes these rows stable (tests/
    index_range.py, F64_ONLY): the f64 pin on both routes, f32 route against route."""
    x = ir.inputs(pkg, "general", where)
    assert x.scene.n_params > 8 and "general" in ir.F64_ONLY
    hip.upload_scene(x.scene)
    ref = ir.expected(oracle, x, "bwd")
    queue = dataclasses.replace(x.rp, bounces_per_launch=1)
    got = render(hip, x, backward=True, f64=True)
    assert got[2]["kernels"]["path"]["launches"] == 1
    pin_f64(x, "general bwd", got, ref)
    pin_f64(x, "general bwd queue", render(hip, x, rp=queue, backward=True, f64=True), ref)
    one, q = render(hip, x, backward=True), render(hip, x, rp=queue, backward=True)
    assert one[2]["kernels"]["path"]["launches"] == 1 and q[2]["kernels"]["path"]["launches"] == 0
    assert np.isfinite(one[1]).all()
    routes_f32(x, "general bwd", one, q)


@pytest.mark.parametrize("family", ["depth4", "general"])
@rows
def test_gradient_image(pkg, hip, oracle, where, family, timed):
    """render_gradient_image of one parameter on cornell and on params12, as test_gradient_image_matches_reference checks one; f32 per
    pixel by check_gradient_image of tests/f32_flips.py on the stable family"""
    x = ir.inputs(pkg, family, where)
    row = where[1]
    hip.upload_scene(x.scene)
    ref = ir.expected(oracle, x, ("gimg", GIMG_PARAM))
    scale = np.abs(ref["grad_image"]).max()
    assert scale > 0
    img, gimg, st = hip.render_gradient_image(x.cam, x.rp, GIMG_PARAM, f64=True)
    assert st["segments"] == ref["stats"]["segments"] and st["capped_paths"] == 0
    np.testing.assert_allclose(gimg[row], ref["grad_image"][row].astype(np.float32), rtol=2e-7, atol=1e-7 * scale)
    np.testing.assert_allclose(img[row], ref["image"][row].astype(np.float32), rtol=2e-7, atol=1e-12)
    assert not gimg[:row].any() and not gimg[row + 1:].any() and not img[:row].any() and not img[row + 1:].any()
    say(where, family + " gimg f64", worst=float(np.abs(gimg[row] - ref["grad_image"][row]).max() / scale))
    img, gimg, st = hip.render_gradient_image(x.cam, x.rp, GIMG_PARAM)
    assert not gimg[:row].any() and not gimg[row + 1:].any() and np.isfinite(gimg).all()
    if family not in ir.F64_ONLY:
        aside, worst = ff.check_gradient_image(img[row][None], gimg[row][None], ref["image"][row][None], ref["grad_image"][row][None],
                                               flip_budget(ir.row_paths(where)))
        say(where, family + " gimg f32", flipped_pixels=aside, worst=worst)
    # its pixel sum is the ordinary gradient of that parameter (f32 on both sides)
    _, grads, _ = hip.render(x.cam, x.rp, backward=True)
    np.testing.assert_allclose(gimg.astype(np.float64).sum((0, 1)) * x.rp.spp, grads[GIMG_PARAM], rtol=1e-5)


# ---- 4: the unbiased operator -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["regen", "specular"])
@rows
def test_unbiased(pkg, hip, oracle, where, family, timed):
    """cornell and cornell_specular, min_bounces = 1, absorb = 0.5, unbiased: k_path_unbiased (bounces_per_launch = 0) and the adjoint-
    round wavefront (1), whose chain carries the key in the bits of a float; path launches as test_unbiased_backward_matches_reference"""
    x = ir.inputs(pkg, family, where)
    hip.upload_scene(x.scene)
    ref = ir.expected(oracle, x, "unbiased")
    queue = dataclasses.replace(x.rp, bounces_per_launch=1)
    got = render(hip, x, backward=True, unbiased=True, f64=True)
    assert got[2]["kernels"]["path"]["launches"] == 1
    pin_f64(x, family + " unbiased one launch", got, ref)
    gq = render(hip, x, rp=queue, backward=True, unbiased=True, f64=True)
    assert gq[2]["kernels"]["path"]["launches"] == 0
    pin_f64(x, family + " unbiased wavefront", gq, ref)
    one, q = render(hip, x, backward=True, unbiased=True), render(hip, x, rp=queue, backward=True, unbiased=True)
    assert one[2]["kernels"]["path"]["launches"] == 1 and q[2]["kernels"]["path"]["launches"] == 0
    routes_f32(x, family + " unbiased", one, q, unbiased=True)
    for what, (_, g, st) in (("one launch", one), ("wavefront", q)):
        err = grad_rel_err(g, ref["grads"])
        say(where, f"{family} unbiased {what} f32", segment_diff=int(st["segments"]) - ref["stats"]["segments"], grad_err=err)
        assert np.isfinite(g).all()
        if family not in ir.F64_ONLY:
            assert err <= UNBIASED_F32, (what, err)


# ---- 5: the queue route, biased ---------------------------------------------------------------------------------------------------
@rows
def test_queue_route(pkg, hip, oracle, where, timed):
    """cornell at fixed depth 4 with bounces_per_launch 1 and 2 and with DRT_RENDER_UNFUSED; loss_l2 with a target image on the tape
    route"""
    x = ir.inputs(pkg, "depth4", where)
    hip.upload_scene(x.scene)
    ref = ir.expected(oracle, x, "bwd")
    for what, rp in (("bpl1", dataclasses.replace(x.rp, bounces_per_launch=1)), ("bpl2", dataclasses.replace(x.rp, bounces_per_launch=2)),
                     ("unfused", dataclasses.replace(x.rp, bounces_per_launch=1, flags=x.rp.flags | pkg.RENDER_UNFUSED))):
        for f64, check in ((True, pin_f64), (False, strict_f32)):
            got = render(hip, x, rp=rp, backward=True, f64=f64)
            assert got[2]["kernels"]["path"]["launches"] == 0 and got[2]["kernels"]["shade"]["launches"] > 0
            assert (got[2]["kernels"]["intersect"]["launches"] > 0) == (what == "unfused")
            check(x, "queue " + what, got, ref)
    loss = ir.expected(oracle, x, "loss_l2")
    tape = dataclasses.replace(x.rp, bounces_per_launch=1)
    tgt = ir.target(where[0], x.seed)
    got = render(hip, x, rp=tape, backward=True, adjoint=tgt, loss_l2=True, f64=True)
    assert got[2]["kernels"]["path"]["launches"] == 0
    pin_f64(x, "queue loss_l2", got, loss)
    got = render(hip, x, rp=tape, backward=True, adjoint=tgt, loss_l2=True)
    assert got[2]["kernels"]["path"]["launches"] == 0
    strict_f32(x, "queue loss_l2", got, loss)


# ---- 6: the mesh ------------------------------------------------------------------------------------------------------------------
@rows
def test_mesh(pkg, hip, oracle, where, timed):
    """mesh10x12, min_bounces = 1, absorb = 0.5: the library's own choice (bounces_per_launch = 0), walk + shade with one bounce per launch
    (1), and the unbiased operator's adjoint rounds with the BVH walk.  The one-launch k_path_mesh is not among them and cannot be: the
    library gives it the frames of at most 2^20 camera samples (DRT_HIP_MESH_PATH_MAX, decided by the size of the FRAME, so that the
    shards of a frame take one route), so no index above 2^20 ever reaches it -- tests/test_gpu_mesh.py covers all it can see.  That a
    frame of this size takes the queue wavefront is asserted."""
    x = ir.inputs(pkg, "mesh", where)
    hip.upload_scene(x.scene)
    ref = ir.expected(oracle, x, "bwd")
    queue = dataclasses.replace(x.rp, bounces_per_launch=1)
    got = render(hip, x, backward=True, f64=True)
    assert got[2]["kernels"]["path"]["launches"] == 0 and got[2]["kernels"]["intersect_mesh"]["launches"] > 0
    pin_f64(x, "mesh the library's choice", got, ref)
    got = render(hip, x, rp=queue, backward=True, f64=True)
    assert got[2]["kernels"]["path"]["launches"] == 0 and got[2]["kernels"]["intersect_mesh"]["launches"] > 0
    pin_f64(x, "mesh walk + shade", got, ref)
    heavy_f32(hip, oracle, x, "mesh the library's choice", ref)
    xq = dataclasses.replace(x, rp=queue)
    heavy_f32(hip, oracle, xq, "mesh walk + shade", ref)
    uref = ir.expected(oracle, x, "unbiased")
    got = render(hip, x, backward=True, unbiased=True, f64=True)
    assert got[2]["kernels"]["path"]["launches"] == 0
    pin_f64(x, "mesh unbiased", got, uref)
    _, g, st = render(hip, x, backward=True, unbiased=True)
    err = grad_rel_err(g, uref["grads"])
    say(where, "mesh unbiased f32", segment_diff=int(st["segments"]) - uref["stats"]["segments"], grad_err=err)
    assert err <= UNBIASED_F32


# ---- three rows in one shard: 2^31 between two pixel groups of one launch -----------------------------------------------------------
@pytest.mark.parametrize("family", ["depth4", "regen"])
def test_three_rows_in_one_shard(pkg, hip, oracle, family, timed):
    """rows 8190 ... 8192 of `top` in one shard (band_rows = 3, n_shards = 5461, shard = 2730): biased on both routes, and the unbiased
    operator's two routes on the regenerating tracer -- f64 against the restatement, f32 route against route"""
    b = ir.BAND3
    where = (b["frame"], b["rows"][1])
    x = ir.inputs(pkg, family, where)
    x.rp = ir.shard_params(pkg, b, x.seed, ir.FAMILIES[family][1])
    assert list(pkg.shard_rows(x.cam.height, b["band_rows"], b["n_shards"], b["shard"])) == list(b["rows"])
    hip.upload_scene(x.scene)
    queue = dataclasses.replace(x.rp, bounces_per_launch=1)
    for unbiased in ((False, True) if family == "regen" else (False,)):
        ref = oracle.render(x.scene, x.cam, x.rp, backward=True, unbiased=unbiased)
        assert not ref["image"][:b["rows"][0]].any() and not ref["image"][b["rows"][-1] + 1:].any()
        tag = f"{family} three rows" + (" unbiased" if unbiased else "")
        for what, rp in (("one launch", x.rp), ("queue", queue)):
            got = render(hip, x, rp=rp, owned=b["rows"], backward=True, unbiased=unbiased, f64=True)
            assert got[2]["kernels"]["path"]["launches"] == (1 if what == "one launch" else 0)
            pin_f64(x, f"{tag} {what}", got, ref, owned=b["rows"])
        one = render(hip, x, owned=b["rows"], backward=True, unbiased=unbiased)
        q = render(hip, x, rp=queue, owned=b["rows"], backward=True, unbiased=unbiased)
        routes_f32(x, tag, one, q, unbiased=unbiased)


# ---- 7: batches at the last row -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["depth4", "general"])
def test_batches_at_the_last_row(pkg, hip, oracle, family, timed):
    """row 16383 of `top` in batches: batch_paths = 100000 cuts the row into pixel batches of 24; batch_paths = 1000 gives one pixel per
    batch and five sample batches, s0 = 1000, 2000, ... -- against the unbatched render by the rule of
    test_deterministic_and_batch_independent, and (f64) against the restatement"""
    x = ir.inputs(pkg, family, ir.TOP_LAST)
    hip.upload_scene(x.scene)
    ref = ir.expected(oracle, x, "bwd")
    a = render(hip, x, backward=True)
    a64 = render(hip, x, backward=True, f64=True)
    for batch, batches in ((100000, 3), (1000, 64 * 5)):
        rp = dataclasses.replace(x.rp, batch_paths=batch)
        c = render(hip, x, rp=rp, backward=True)
        assert c[2]["segments"] == a[2]["segments"] and c[2]["batches"] == batches
        np.testing.assert_allclose(c[0], a[0], rtol=1e-6, atol=1e-9)
        np.testing.assert_allclose(c[1], a[1], rtol=1e-9)
        c64 = render(hip, x, rp=rp, backward=True, f64=True)
        assert c64[2]["batches"] == batches
        pin_f64(x, f"{family} batch_paths {batch}", c64, ref)
        say(x.where, f"{family} batch_paths {batch}", batches=c[2]["batches"], f32_grad_diff=grad_rel_err(c[1], a[1]),
            f64_grad_diff=grad_rel_err(c64[1], a64[1]))


# ---- 9: the limit itself ------------------------------------------------------------------------------------------------------------
TOO_MANY = "render: more than 2^32 camera samples in one frame (width x height x spp)"


def test_the_limit_itself(pkg, oracle, timed):
    """one context: 64 x 16384 x 4096 = 2^32 is accepted (its last row); 64 x 16384 x 4097 and 65536 x 65536 x 2 are refused with
    DRT_ERR_INVALID and the complete text, and the context renders the fixed-depth case correctly afterwards; a shard that owns no row
    returns status 0, zero paths and segments and zero gradients"""
    r = pkg.HipRenderer(0)
    try:
        x = ir.inputs(pkg, "depth4", ir.TOP_LAST)
        assert x.cam.width * x.cam.height * x.rp.spp == 2 ** 32
        r.upload_scene(x.scene)
        ref = ir.expected(oracle, x, "bwd")
        pin_f64(x, "limit: 2^32 accepted", render(r, x, backward=True, f64=True), ref)
        for cam, spp in ((x.cam, 4097), (pkg.Camera(65536, 65536).look_at(ir.EYE, ir.AT), 2)):
            rp = dataclasses.replace(x.rp, spp=spp, n_shards=cam.height, shard=cam.height - 1)
            assert cam.width * cam.height * spp > 2 ** 32
            desc, cd = rp.to_desc(), cam.to_desc()
            import ctypes as C
            rc = r.lib.drt_hip_render(r.ctx, C.byref(cd), C.byref(desc), None, None, None, None)
            assert pkg.STATUS_NAMES[rc] == "DRT_ERR_INVALID"
            assert r.lib.drt_hip_last_error(r.ctx).decode() == TOO_MANY
        pin_f64(x, "limit: after the refusals", render(r, x, backward=True, f64=True), ref)
        strict_f32(x, "limit: after the refusals", render(r, x, backward=True), ref)
        e = ir.EMPTY_SHARD
        rp = ir.shard_params(pkg, e, x.seed, ir.FAMILIES["depth4"][1])
        assert len(pkg.shard_rows(x.cam.height, e["band_rows"], e["n_shards"], e["shard"])) == 0
        for f64 in (True, False):
            img, grads, st = render(r, x, rp=rp, owned=(), backward=True, f64=f64)
            assert st["paths"] == 0 and st["segments"] == 0 and not grads.any()
    finally:
        r.close()


# ---- 8: the derived forms on the largest frame they accept --------------------------------------------------------------------------
class RowOutputs:
    """one case's outputs as tests/test_gpu_launch_geometry.py's checks read them, every frame-sized array cut to the shard's row (the
    rows the shard does not own are checked to be exactly zero when an output is put in)"""
    where = ("cornell", "depth4", ir.HALF_ROW)

    def __init__(self, cam, row):
        self.out, self.frame, self.row = {}, (cam.height, cam.width, 3), row

    def put(self, call, f64, **fields):
        import geometry_child as gc
        for k, v in fields.items():
            v = gc.stats_row(v) if k == "stats" else np.asarray(v)
            if v.shape[-3:] == self.frame:
                assert not v[..., :self.row, :, :].any() and not v[..., self.row + 1:, :, :].any(), (call, k, "a row the shard does not own")
                v = v[..., self.row:self.row + 1, :, :]
            self.out[(call, f64, k)] = v

    def get(self, call, f64, field):
        return self.out[(call, f64, field)]

    def stat(self, call, f64, field):
        import geometry_child as gc
        return int(self.out[(call, f64, "stats")][gc.STATS.index(field)])


def test_derived_forms_on_the_largest_frame_they_accept(pkg, hip, oracle, timed):
    """`half` (64 x 8192 x 4095 = 2,146,959,360 <= 2^31 - 1 samples), its last row (quiet-NaN patterns), cornell at depth 4, f64 and f32:
    render_tangent, render_tangents (K = 3), render_normal_equations (with its Jacobian images), render_param_sets (3 sets and a target),
    render_param_sets_grad (3 sets, an adjoint each).  Expected values as the forms' own files compute them -- J v from the restatement's
    per-parameter gradient images, A, b and loss from those, set k from the restatement with P_k installed -- through the checks and
    bounds of tests/test_gpu_launch_geometry.py (derived_f64, derived_f32), on the shard's row."""
    import types

    import test_gpu_launch_geometry as lg
    from test_gpu_cross import target_for
    from test_gpu_sets_grad import four_sets, with_params
    from test_gpu_tangents import directions
    x = ir.inputs(pkg, "depth4", ir.HALF_ROW)
    scene, cam, rp, row = x.scene, x.cam, x.rp, x.where[1]
    assert cam.width * cam.height * rp.spp <= 2 ** 31 - 1 < cam.width * cam.height * (rp.spp + 1)
    P, W = four_sets(scene, cam, 31)
    P, W, V, target = P[:3], W[:3], directions(scene, 3, 23), target_for(cam)
    cut = slice(row, row + 1)
    fwd = ir.expected(oracle, x, "fwd")
    J = np.stack([np.array(ir.expected(oracle, x, ("gimg", p))["grad_image"][cut]) for p in range(scene.n_params)])
    sets = [oracle.render(with_params(scene, P[k]), cam, rp, backward=True, adjoint=W[k]) for k in range(3)]
    assert fwd["stats"]["deepest"] < 64
    E = {"x": types.SimpleNamespace(target=target[cut]), "image": fwd["image"][cut], "segments": fwd["stats"]["segments"], "capped": 0,
         "J": J, "T": np.einsum("phwc,kpc->khwc", J, V), "set_images": np.stack([r["image"][cut] for r in sets]),
         "set_grads": np.stack([r["grads"] for r in sets])}
    hip.upload_scene(scene)
    c = RowOutputs(cam, row)
    for f64 in (True, False):
        img, timg, st = hip.render_tangent(cam, rp, V[0], f64=f64)
        c.put("tangent", f64, image=img, tangent=timg, stats=st)
        img, timg, st = hip.render_tangents(cam, rp, V, f64=f64)
        c.put("tangents", f64, image=img, tangents=timg, stats=st)
        r = hip.render_normal_equations(cam, rp, target=target, f64=f64, jacobian=True)
        c.put("neq", f64, image=r["image"], A=r["A"], b=r["b"], loss=r["loss"], jacobian=r["jacobian"], stats=r["stats"])
        r = hip.render_param_sets(cam, rp, P, target=target, f64=f64, double=f64)
        c.put("sets", f64, images=r["images"], loss=r["loss"], stats=r["stats"])
        r = hip.render_param_sets_grad(cam, rp, P, W, f64=f64)
        c.put("sets_grad", f64, grads=r["grads"], stats=r["stats"])
    calls = ("tangent", "tangents", "neq", "sets", "sets_grad")
    what = ("half", "cornell", "depth4", ir.HALF_ROW)
    lg.derived_f64("half", c, E, calls, what)
    print(f"index_range half-{row} derived forms f64: worst error against the restatement {lg._worst.get('half', float('nan')):.3e}")
    failures = lg.Failures()
    lg.derived_f32(failures, c, E, calls, what, ir.row_paths(ir.HALF_ROW))
    failures.raise_all()
