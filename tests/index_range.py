"""Frames whose camera-sample indices reach the top of the 32-bit range -- the case tables of tests/test_gpu_index_range.py and of its
CPU companion tests/test_index_range_inputs.py.

A camera sample's identity is its index pixel * spp + sample: the RNG key of its path.  drt_hip_render accepts a frame of up to exactly
2^32 samples, the derived entry points one of up to 2^31 - 1.  A render takes (shard, n_shards, band_rows), traces only the shard's rows
with the FRAME's pixel numbers and copies back only them: one image row of a 2^32-sample frame is a few hundred thousand paths, and the
fp64 restatement (oracle.render) honours the same three fields with a 64-bit path index.

On the adjoint-round wavefront the key travels in the bits of a float (csrc/drt_chain.h, pid_pack); PATTERNS names what those bits are
as an f32 value, band by band.

A plain module, like tests/mesh_families.py."""
import dataclasses
import types

import numpy as np

# name -> (width, height, spp, the most samples the entry points under test accept)
FRAMES = {"top": (64, 16384, 4096, 2 ** 32),          # exactly 2^32 samples
          "odd": (40, 35779, 3001, 2 ** 32),          # 4,294,911,160: nothing a power of two
          "half": (64, 8192, 4095, 2 ** 31 - 1)}      # 2,146,959,360: the largest frame of this shape the derived forms accept
EYE, AT = (0.1, 0.0, -0.2), (0, 0.2, 1)

# (frame, row) -> (first index, last index, what the indices are).  One render per row: band_rows = 1, n_shards = H, shard = row.
ROWS = {("top", 0): (0, 262143, "control: what every other test covers"),
        ("top", 8160): (2139095040, 2139357183, "+Inf, then signalling NaNs"),
        ("top", 8191): (2147221504, 2 ** 31 - 1, "quiet NaNs, up to 2^31 - 1"),
        ("top", 8192): (2 ** 31, 2 ** 31 + 262143, "the sign bit: -0, negative denormals"),
        ("top", 16383): (2 ** 32 - 262144, 2 ** 32 - 1, "negative NaNs, up to 0xFFFFFFFF"),
        ("odd", 17889): (2147395560, 2147515599, "2^31 inside the samples of pixel 29 of the row"),
        ("half", 8191): (2146697280, 2146959359, "quiet NaNs: the last row of the derived forms' largest frame")}
RENDER_ROWS = [k for k in ROWS if k[0] != "half"]       # every case runs at these
HALF_ROW = ("half", 8191)
TOP_LAST = ("top", 16383)
# three rows in one shard of `top`: rows 8190 ... 8192, 2^31 between two pixel groups of one launch
BAND3 = dict(frame="top", band_rows=3, n_shards=5461, shard=2730, rows=(8190, 8191, 8192))
# a shard of `top` that owns no row (16384 rows are 8192 bands of two)
EMPTY_SHARD = dict(frame="top", band_rows=2, n_shards=16384, shard=9000)

# the float whose bits are the index, band by band: (first index, last index, name)
PATTERNS = ((0, 0, "+0"), (1, 0x007FFFFF, "positive denormal"), (0x00800000, 0x7F7FFFFF, "positive number"), (0x7F800000, 0x7F800000, "+Inf"),
            (0x7F800001, 0x7FBFFFFF, "signalling NaN"), (0x7FC00000, 0x7FFFFFFF, "quiet NaN"), (0x80000000, 0x80000000, "-0"),
            (0x80000001, 0x807FFFFF, "negative denormal"), (0x80800000, 0xFF7FFFFF, "negative number"), (0xFF800000, 0xFF800000, "-Inf"),
            (0xFF800001, 0xFFFFFFFF, "negative NaN"))
# the patterns each row's indices are, in index order (tests/test_index_range_inputs.py derives them from PATTERNS)
ROW_PATTERNS = {("top", 0): ("+0", "positive denormal"),
                ("top", 8160): ("+Inf", "signalling NaN"),
                ("top", 8191): ("quiet NaN",),
                ("top", 8192): ("-0", "negative denormal"),
                ("top", 16383): ("negative NaN",),
                ("odd", 17889): ("quiet NaN", "-0", "negative denormal"),
                ("half", 8191): ("quiet NaN",)}

# the case families: name -> (scene, tracer).  The f32 bound of a family: GRAD_TOL on the reference's scenes, GRAD_TOL_HEAVY with the
# flip-aware check on the random room and on the mesh (tests/test_gpu_parity.py).
FAMILIES = {"depth4": ("cornell", dict(min_bounces=4, absorb=1.0)),            # k_path_lean and the role kernels; f64: the literal k_path
            "regen": ("cornell", dict(min_bounces=1, absorb=0.5)),             # the regenerating form
            "general": ("params12", dict(min_bounces=3, absorb=0.3)),          # history words, per-wave tables
            "specular": ("cornell_specular", dict(min_bounces=1, absorb=0.5)),  # with `regen`: the unbiased operator's two scenes
            "mesh": ("mesh10x12", dict(min_bounces=1, absorb=0.5))}            # walk + shade, adjoint rounds with the BVH walk (k_path_mesh: frames of <= 2^20 samples only)
HEAVY = ("general", "mesh")
UNBIASED = ("regen", "specular", "mesh")

# The seed of every (family, frame, row): the first from 1 upwards at which the frame is STABLE by the stand-in criterion of
# tests/f32_flips.py (three jittered fp64 renders, at most one pixel set aside, corrected gradient error a tenth of the bound; under the
# unbiased operator as well: no pixel moved and the gradient by less than UNBIASED_MOVE) and no pixel's specular lobe is conditioned worse
# than the f32 pixel bound allows (lobe_conditioning of tests/test_gpu_launch_geometry.py) -- decided by the restatement alone, on the
# CPU, by tools of this module (first_stable_seed); tests/test_index_range_inputs.py re-derives that each recorded seed is stable.
# 1 everywhere but here:
SEEDS = {("depth4", "top", 0): 3, ("depth4", "top", 16383): 2,
         ("regen", "top", 0): 4, ("regen", "top", 8160): 4, ("regen", "top", 8191): 2, ("regen", "top", 16383): 7,
         ("mesh", "top", 0): 2, ("mesh", "top", 8160): 5, ("mesh", "top", 8191): 2}
# The families that NO seed up to SEED_LIMIT makes stable, at any row: they keep their f64 pin (1e-9, equal segments) and, in f32, are
# compared route against route.  What rejects them is the depth of the pixels, not the index: at 3001 ... 4096 samples a pixel ONE
# flipped path moves a pixel of a heavy-tailed room beyond PIXEL_TOL of the largest value and yet by far less than FLIP_MIN_REL of its own
# value (general: 4e-4 ... 7e-4 of it), which the flip-aware check does not excuse; and among a pixel's thousands of glossy bounces one always
# has its half vector within a fraction of a degree of the normal (specular: the conditioning rule is exceeded 40 ... 9600 times over
# at the few seeds where the unbiased operator's gradient does not move).
SEED_LIMIT = 32
F64_ONLY = ("general", "specular")


def seed_of(family, where):
    return SEEDS.get((family,) + tuple(where), 1)


def interval(width, height, spp, row, rows=1):
    """the first and the last sample index of `rows` image rows from `row` on"""
    assert 0 <= row and row + rows <= height
    return row * width * spp, (row + rows) * width * spp - 1


def pattern_of(index):
    """the name of the f32 value whose bits are `index`"""
    (name,) = [n for lo, hi, n in PATTERNS if lo <= index <= hi]
    return name


def patterns_between(first, last):
    """the patterns of first ... last in index order"""
    return tuple(n for lo, hi, n in PATTERNS if lo <= last and first <= hi)


def camera(pkg, frame):
    w, h, _, _ = FRAMES[frame]
    return pkg.Camera(w, h).look_at(EYE, AT)


def row_params(pkg, frame, row, seed, tracer, **kw):
    """the render of one row: band_rows = 1, n_shards = H, shard = row"""
    _, h, spp, _ = FRAMES[frame]
    return pkg.RenderParams(spp=spp, seed=seed, shard=row, n_shards=h, band_rows=1, **tracer, **kw)


def shard_params(pkg, what, seed, tracer):
    """BAND3 or EMPTY_SHARD"""
    return pkg.RenderParams(spp=FRAMES[what["frame"]][2], seed=seed, shard=what["shard"], n_shards=what["n_shards"],
                            band_rows=what["band_rows"], **tracer)


def adjoint(frame, seed):
    w, h, _, _ = FRAMES[frame]
    return np.random.RandomState(seed).uniform(-1, 2, (h, w, 3)).astype(np.float32)


def target(frame, seed):
    """the target image of loss_l2, as conftest.case_inputs draws one"""
    w, h, _, _ = FRAMES[frame]
    return np.random.RandomState(seed).uniform(0, 0.6, (h, w, 3)).astype(np.float32)


def row_paths(where):
    w, _, spp, _ = FRAMES[where[0]]
    return w * spp


@dataclasses.dataclass
class Inputs:
    family: str
    where: tuple
    scene: object
    cam: object
    rp: object
    seed: int


def inputs(pkg, family, where, **kw):
    name, tracer = FAMILIES[family]
    seed = seed_of(family, where)
    return Inputs(family, tuple(where), pkg.scene_by_name(name), camera(pkg, where[0]), row_params(pkg, where[0], where[1], seed, tracer, **kw), seed)


# ---- the restatement's values, computed once and shared (read-only) ---------------------------------------------------------------
_expected = {}
_adjoints = {}


def adjoint_of(x):
    key = (x.where[0], x.seed)
    if key not in _adjoints:
        _adjoints[key] = adjoint(*key)
        _adjoints[key].setflags(write=False)
    return _adjoints[key]


def expected(oracle, x, what):
    """what: "fwd" | "bwd" | "adj" (backward with the adjoint image) | "unbiased" | "loss_l2" | ("gimg", p) -> the restatement's render"""
    key = (x.family, x.where, x.seed, what)
    if key not in _expected:
        if what == "fwd":
            r = oracle.render(x.scene, x.cam, x.rp)
        elif what == "bwd":
            r = oracle.render(x.scene, x.cam, x.rp, backward=True)
        elif what == "adj":
            r = oracle.render(x.scene, x.cam, x.rp, backward=True, adjoint=adjoint_of(x))
        elif what == "unbiased":
            r = oracle.render(x.scene, x.cam, x.rp, backward=True, unbiased=True)
        elif what == "loss_l2":
            r = oracle.render(x.scene, x.cam, x.rp, backward=True, adjoint=target(x.where[0], x.seed), loss_l2=True)
        else:
            r = oracle.render(x.scene, x.cam, x.rp, backward=True, grad_image_param=what[1])
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _expected[key] = r
    return _expected[key]


def row_of(image, where):
    """the one row of a frame-sized image that a row's render owns, and whether every other row is exactly zero"""
    row = where[1]
    return image[row], not image[:row].any() and not image[row + 1:].any()


# ---- which seed: decided on the CPU -----------------------------------------------------------------------------------------------
def lobe_lost(oracle, x, images):
    """the launch-geometry test's conditioning rule on one row: what four roundings of the specular lobe's cancellation cost the worst
    pixel of each image, in units of the f32 pixel bound (<= 1: inside the comparison's domain)"""
    from test_gpu_launch_geometry import F32_EPS, lobe_conditioning
    from test_gpu_parity import PIXEL_TOL
    first, last = interval(x.cam.width, x.cam.height, x.rp.spp, x.where[1])
    kappa = lobe_conditioning(oracle, types.SimpleNamespace(scene=x.scene, cam=x.cam, rp=x.rp), max_vertices=(last - first + 1) * 64)
    return max(float((4 * F32_EPS * kappa[..., None] * np.abs(v)).max() / (PIXEL_TOL * np.abs(v).max())) for v in images)


def stable_record(oracle, x):
    """-> (stable, a dict of what decided it) for one (family, row) at x.seed"""
    import f32_flips as ff
    from test_gpu_parity import GRAD_TOL, GRAD_TOL_HEAVY
    tol = GRAD_TOL_HEAVY if x.family in HEAVY else GRAD_TOL
    recs = ff.standin_records(oracle, x.scene, x.cam, x.rp, None, tol, max_bad=1)
    rec = {"set_aside": [None if isinstance(r, AssertionError) else r["set_aside"] for r in recs],
           "corrected": [None if isinstance(r, AssertionError) else r["grad_err_corrected"] for r in recs]}
    ok = all(not isinstance(r, AssertionError) and r["grad_err_corrected"] <= tol / 10 for r in recs)
    if ok and x.family in UNBIASED:
        px, move = ff.unbiased_move(oracle, x.scene, x.cam, x.rp, None)
        rec.update(unbiased_pixels=px, unbiased_move=move)
        ok = px == 0 and move < ff.UNBIASED_MOVE
    if ok and any(m[0] == 1 for m in x.scene.materials):
        rec["lobe"] = lobe_lost(oracle, x, [expected(oracle, x, "fwd")["image"]])
        ok = rec["lobe"] <= 1.0
    return ok, rec


def first_stable_seed(pkg, oracle, family, where):
    """the first seed from 1 to SEED_LIMIT at which (family, row) is stable, or None"""
    for seed in range(1, SEED_LIMIT + 1):
        x = inputs(pkg, family, where)
        x.seed, x.rp = seed, dataclasses.replace(x.rp, seed=seed)
        if stable_record(oracle, x)[0]:
            return seed
    return None
