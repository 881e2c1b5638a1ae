"""Mesh families for tests/test_mesh_families.py (CPU) and tests/test_gpu_mesh_geometry.py (GPU); a helper, not a collected test.  numpy only.

Every triangle the device intersected in a test used to belong to one smooth, closed, well-tessellated surface seen from outside
(displaced_sphere_mesh).  The families here are what that surface is not: coincident copies (every hit an exact tie, traversal stacks
deeper than the 16 entries k_path_mesh keeps in LDS), random slivers with degenerate faces among them, an open sheet seen from both sides,
meshes that emit, two meshes with the analytic shapes between them, nested scales (the build that meets the stack bound).  All of them are
the reference's Cornell box (pkg.cornell_box()) with something replaced; coordinates lie inside the room: x, y in (-3, 3), z in (0, 6), the
camera at the origin looking along +z.

Besides the scenes: the rays the CPU tests feed tests/cpp/bvh_walk_replay.cpp (pixel centres of a frame, seeded wall-to-mesh rays, each
with its closest analytic hit) and the file format of that program."""
import numpy as np

SHAPE_PLANE, SHAPE_SPHERE, SHAPE_MESH = 0, 1, 2
WHITE_MATERIAL, SPECULAR_MATERIAL, EMITTER = 2, 3, 0      # cornell_box(): diffuse_white, specular_white (exponent 30), the light's emitter
QUAD = np.array([(-0.9, -2.0, 3.4), (0.9, -2.0, 3.0), (0.9, -0.2, 3.1), (-0.9, -0.2, 3.5)])     # one tilted quad in front of the camera
N_DEGENERATE = 8


def _replace_shape0(pkg, s, v, idx, material, emitter=-1, face_material=None):
    """the mesh (v, idx) in the place of sphere_front"""
    s.mesh(v, idx, material, emitter, face_material=face_material)
    s.shapes[0] = s.shapes.pop()
    return s


def deck(pkg, n, last=False):
    """n coincident copies of QUAD (own vertices, two triangles each) in the place of sphere_front.  One copy -- the first, or (`last`)
    the last -- is diffuse on a parameter `first` of its own, the others are white: the reference's linear scan keeps the FIRST of equal
    hits (pathtracer.hpp:80), so `deck` shows `first`'s colour and carries its gradient, `deck_last` is a white quad and `first` gets
    exactly nothing."""
    s = pkg.cornell_box()
    odd = s.diffuse(s.parameter((0.7, 0.2, 0.1), True, "first"))
    v = np.tile(QUAD, (n, 1))
    base = 4 * np.arange(n)[:, None]
    idx = np.concatenate([base + np.array([0, 1, 2]), base + np.array([0, 2, 3])], 1).reshape(-1, 3)
    fm = np.full(2 * n, WHITE_MATERIAL, dtype=np.int32)
    k = n - 1 if last else 0
    fm[2 * k: 2 * k + 2] = odd
    return _replace_shape0(pkg, s, v, idx, WHITE_MATERIAL, face_material=fm)


def deck_last(pkg, n):
    return deck(pkg, n, last=True)


def two_meshes(pkg, reverse=False):
    """Shape 0 is a mesh of one quad with material A; the LAST shape, behind the light sphere, a second mesh of the same coordinates with
    material B; every analytic shape lies between them in scene order.  One BVH holds both, and shape 0's faces win every hit: A carries
    the quad's gradient, B exactly nothing.  `reverse`: the materials swapped."""
    s = pkg.cornell_box()
    A = s.diffuse(s.parameter((0.7, 0.2, 0.1), True, "A"))
    B = s.diffuse(s.parameter((0.1, 0.3, 0.8), True, "B"))
    idx = np.array([(0, 1, 2), (0, 2, 3)])
    _replace_shape0(pkg, s, QUAD, idx, B if reverse else A)
    s.mesh(QUAD.copy(), idx, A if reverse else B)
    return s


def two_meshes_reversed(pkg):
    return two_meshes(pkg, reverse=True)


def sliver_triangles(n, seed):
    """n slivers -- a, b uniform in a 2.6-wide cube centred at (0, -1, 3.5), c = a + 0.01 u -- and N_DEGENERATE faces with a repeated vertex
    index ((i, i, j) and (i, j, i): an edge of exactly zero, so det == 0 exactly and no ray ever hits them; the upload stores a NaN normal)"""
    rs = np.random.RandomState(seed)
    a = rs.uniform(-1.3, 1.3, (n, 3)) + np.array([0.0, -1.0, 3.5])
    b = rs.uniform(-1.3, 1.3, (n, 3)) + np.array([0.0, -1.0, 3.5])
    c = a + 0.01 * rs.uniform(-1.0, 1.0, (n, 3))
    v = np.stack([a, b, c], 1).reshape(-1, 3)
    idx = np.arange(3 * n).reshape(n, 3)
    where = rs.choice(n, N_DEGENERATE, replace=False)
    deg = np.array([(3 * t, 3 * t, 3 * t + 1) if k % 2 == 0 else (3 * t, 3 * t + 1, 3 * t) for k, t in enumerate(where)])
    # (the degenerate faces stand in the middle of the face list, not behind it)
    idx = np.concatenate([idx[: n // 2], deg, idx[n // 2:]])
    return v, idx


def slivers(pkg, n, seed, face_params=0):
    """sliver_triangles in the place of sphere_front, white; face_params > 0: that many diffuse albedos of their own handed to the faces
    round-robin, as cornell_with_mesh(per_face_params=...) does (12 of them: 16 parameters, the general gradient form, whose history
    shares an allocation with the traversal stacks' overflow)"""
    s = pkg.cornell_box()
    v, idx = sliver_triangles(n, seed)
    fm = None
    if face_params > 0:
        rs = np.random.RandomState(seed + 1)
        mats = [s.diffuse(s.parameter(rs.uniform(0.2, 0.9, 3), True, f"face{i}")) for i in range(face_params)]
        fm = np.array([mats[t % face_params] for t in range(len(idx))], dtype=np.int32)
    return _replace_shape0(pkg, s, v, idx, WHITE_MATERIAL, face_material=fm)


def slivers_faces(pkg, n, seed):
    return slivers(pkg, n, seed, face_params=12)


def sheet_triangles(cells=12):
    """a sloping sheet of cells x cells quads from the ground, (+-1.5, -3, 2), up to (+-1.5, -1, 4.6): the camera sees one side, the paths
    that come back from the wall behind it the other"""
    u, w = np.meshgrid(np.linspace(0, 1, cells + 1), np.linspace(0, 1, cells + 1), indexing="ij")
    v = np.stack([-1.5 + 3.0 * u, -3.0 + 2.0 * w, 2.0 + 2.6 * w], -1).reshape(-1, 3)
    at = lambda i, j: i * (cells + 1) + j
    idx = []
    for i in range(cells):
        for j in range(cells):
            a, b, c, d = at(i, j), at(i + 1, j), at(i + 1, j + 1), at(i, j + 1)
            idx += [(a, b, c), (a, c, d)]
    return v, np.array(idx)


def open_sheet(pkg, glow=False):
    """sheet_triangles in the place of sphere_front, its faces in turn diffuse and specular (both on `white`).  An open surface: paths meet
    its faces from behind too, where the contract is a two-sided hit with the normal as stored.  `glow`: the sheet also
    emits, on a small parameter `glow` of its own (what cornell_box(emissive_wall=True) does for a plane)."""
    s = pkg.cornell_box()
    v, idx = sheet_triangles()
    fm = np.where(np.arange(len(idx)) % 2 == 0, WHITE_MATERIAL, SPECULAR_MATERIAL).astype(np.int32)
    emitter = s.area_emitter(s.parameter((0.05, 0.1, 0.2), True, "glow")) if glow else -1
    return _replace_shape0(pkg, s, v, idx, WHITE_MATERIAL, emitter, face_material=fm)


def glowing_sheet(pkg):
    return open_sheet(pkg, glow=True)


def quad_light(pkg):
    """the light sphere replaced by a two-triangle mesh under the ceiling: no BxDF (material -1), the scene's emitter"""
    s = pkg.cornell_box()
    s.shapes.pop()
    v = np.array([(-1.0, 2.9, 2.0), (1.0, 2.9, 2.0), (1.0, 2.9, 4.0), (-1.0, 2.9, 4.0)])
    s.mesh(v, np.array([(0, 1, 2), (0, 2, 3)]), -1, EMITTER)
    return s


def nested_triangles(n, seed):
    """tests/cpp/bvh_kat.cpp's `nested` soup -- clusters of clusters, scale 4^-level, centres drifting along a line -- scaled into the room"""
    rs = np.random.RandomState(seed)
    level = np.arange(n) % 7
    sc = 0.25 ** level
    u = rs.uniform(-1.0, 1.0, (n, 3, 3))
    v0 = 3.0 * (1.0 - sc)[:, None] + sc[:, None] * u[:, 0]
    v0[:, 1:] += 0.1 * level[:, None]
    e1, e2 = 0.05 * sc[:, None] * u[:, 1], 0.05 * sc[:, None] * u[:, 2]
    v = np.stack([v0, v0 + e1, v0 + e2], 1).reshape(-1, 3)
    v = (v + 1.0) * 0.55 + np.array([-1.5, -2.5, 2.2])
    return v, np.arange(3 * n).reshape(n, 3)


def nested(pkg, n, seed):
    s = pkg.cornell_box()
    v, idx = nested_triangles(n, seed)
    return _replace_shape0(pkg, s, v, idx, WHITE_MATERIAL)


def control(pkg):
    """the mesh every earlier test used (the control of the input conditions)"""
    return pkg.cornell_with_mesh(40, 40)


# ---- the sizes and seeds the tests use.  Chosen so that the input conditions of tests/test_mesh_families.py hold; a family that misses
# one gets another size or seed HERE, the thresholds there stay
DECK_N = 1024
DECK_SMALL_N = 256
SLIVERS_N, SLIVERS_SEED = 1000, 3          # the first seed from 1 upwards with 15 primary and 500 secondary rays beyond the LDS stack
NESTED_N, NESTED_SEED = 40000, 2            # stack_need meets the bound of 30 after a first build that needed 31

FAMILIES = {
    "deck": lambda pkg: deck(pkg, DECK_N),
    "deck_last": lambda pkg: deck_last(pkg, DECK_N),
    "deck_small": lambda pkg: deck(pkg, DECK_SMALL_N),
    "two_meshes": two_meshes,
    "two_meshes_reversed": two_meshes_reversed,
    "slivers": lambda pkg: slivers(pkg, SLIVERS_N, SLIVERS_SEED),
    "slivers_faces": lambda pkg: slivers_faces(pkg, SLIVERS_N, SLIVERS_SEED),
    "open_sheet": open_sheet,
    "glowing_sheet": glowing_sheet,
    "quad_light": quad_light,
    "nested": lambda pkg: nested(pkg, NESTED_N, NESTED_SEED),
    "control": control,
}
# the parameters each family is about: (those that must carry a gradient, those that must get exactly none)
ABOUT = {
    "deck": (("first",), ()), "deck_small": (("first",), ()), "deck_last": ((), ("first",)),
    "two_meshes": (("A",), ("B",)), "two_meshes_reversed": (("B",), ("A",)),
    "slivers_faces": (tuple(f"face{i}" for i in range(12)), ()),
    "glowing_sheet": (("glow",), ()), "quad_light": (("emission",), ()),
}



# ---- the GPU cases (tests/test_gpu_mesh_geometry.py renders them, tests/test_mesh_families.py checks their inputs on the CPU)
FRAME, SPP, SEED = (24, 20), 2, 3
TRACERS = (dict(min_bounces=4, absorb=1.0), dict(min_bounces=1, absorb=0.5))
BASE = ("deck", "deck_last", "two_meshes", "two_meshes_reversed", "slivers", "open_sheet", "glowing_sheet", "quad_light", "nested")
OVERFLOW = ("deck", "slivers")                  # the families whose rays hold more entries than the LDS part of k_path_mesh's stack
TIES = ("deck", "deck_last", "deck_small", "two_meshes", "two_meshes_reversed")      # every ray that hits meets an exact tie
UNBIASED = ("deck_small", "slivers")            # under the unbiased operator, 1 spp
SLIVER_FAMILIES = ("slivers", "slivers_faces")
UNBIASED_TRACER, UNBIASED_SEED = 1, 4           # (the first seed from 3 upwards at which a resampled suffix carries light to `first`: the quad faces away from the light)
FACES_FRAME, FACES_SPP = (64, 48), 4            # slivers_faces: the smallest of the frames tried at which both tracers reach all 12 face albedos


def family(pkg, name):
    return FAMILIES[name](pkg)


def camera(pkg, frame=FRAME):
    return pkg.cornell_camera(*frame)


def render_params(pkg, tracer, spp=SPP, seed=SEED, **kw):
    return pkg.RenderParams(spp=spp, seed=seed, **TRACERS[tracer], **kw)


# ---- the scene as the device flattens it (drt_scene.h, upload_scene) ---------------------------------------------------------------
def flat_triangles(scene):
    """-> (vertices f64 [n, 3, 3], flat index int64 [n], shape index int64 [n]): every triangle of every mesh shape in scene order, with
    its position in the flattened scene (an analytic shape counts one, a mesh its triangles: the tie order)"""
    tris, flats, shapes = [], [], []
    flat = 0
    for i, (t, m, e, p) in enumerate(scene.shapes):
        if t != SHAPE_MESH:
            flat += 1
            continue
        v, idx, _ = scene.meshes[int(p[0])]
        tris.append(v[idx.astype(np.int64)])
        flats.append(flat + np.arange(len(idx)))
        shapes.append(np.full(len(idx), i))
        flat += len(idx)
    return np.concatenate(tris), np.concatenate(flats), np.concatenate(shapes)


def analytic_extent(scene):
    """the largest distance from the origin among the analytic shapes, as upload_scene's pad rule measures it (drt_scene.h)"""
    extent = 0.0
    for t, m, e, p in scene.shapes:
        if t == SHAPE_PLANE:
            nn = np.sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2])
            if nn > 0:
                extent = max(extent, abs(p[3]) / nn)
        elif t == SHAPE_SPHERE:
            extent = max(extent, np.sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]) + abs(p[3]))
    return extent


def analytic_hit(scene, o, d):
    """closest plane / sphere of the scene for rays (o, d) [n, 3] -> (t [n] (inf: none), flat index [n] (-1: none)); the predicates of
    shape.hpp:49-59, 78-103 (t > 0, the first shape keeps a tie)"""
    n = len(o)
    tmin, best = np.full(n, np.inf), np.full(n, -1, dtype=np.int64)
    flat = 0
    with np.errstate(all="ignore"):
        for ty, m, e, p in scene.shapes:
            if ty == SHAPE_MESH:
                flat += len(scene.meshes[int(p[0])][1])
                continue
            if ty == SHAPE_PLANE:
                nrm = np.array(p[:3])
                t = (o @ nrm - p[3]) / -(d @ nrm)
                ok = t > 0
            else:
                oc = o - np.array(p[:3])
                b = 2.0 * (oc * d).sum(1)
                c = (oc * oc).sum(1) - p[3] * p[3]
                disc = b * b - 4.0 * c
                sq = np.sqrt(np.maximum(disc, 0.0))
                t1, t2 = (-b - sq) * 0.5, (-b + sq) * 0.5
                t = np.where(t1 > 0, t1, t2)
                ok = (disc >= 0) & (t > 0)
            take = ok & (t < tmin)
            tmin[take], best[take] = t[take], flat
            flat += 1
    return tmin, best


def primary_rays(cam):
    """the rays through the pixel centres of `cam` (camera.hpp:51-60 with both draws at 1/2) -> (o [n, 3], d [n, 3]), row-major"""
    x, y = np.meshgrid(np.arange(cam.width), np.arange(cam.height))
    s, t = (x.reshape(-1) + 0.5) / cam.width, (y.reshape(-1) + 0.5) / cam.height
    th = np.tan(cam.vfov / 2.0)
    d = (np.array(cam.forward)[None] + np.array(cam.right)[None] * ((2 * s - 1) * (cam.width / cam.height) * th)[:, None]
         - np.array(cam.up)[None] * ((2 * t - 1) * th)[:, None])
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.tile(np.array(cam.eye, dtype=np.float64), (len(d), 1)), d


def wall_rays(scene, n, seed):
    """n rays from random points just inside the room's six walls towards random points of the mesh's bounding box: what a path's second
    and later segments look like from the mesh's side (incoherent, from every direction)"""
    rs = np.random.RandomState(seed)
    tris, _, _ = flat_triangles(scene)
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    room_lo, room_hi = np.array([-2.9, -2.9, 0.1]), np.array([2.9, 2.9, 5.9])
    o = rs.uniform(room_lo, room_hi, (n, 3))
    axis, side = rs.randint(0, 3, n), rs.randint(0, 2, n)
    o[np.arange(n), axis] = np.where(side == 0, room_lo[axis], room_hi[axis])
    target = rs.uniform(lo, hi, (n, 3))
    d = target - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o, d


# ---- tests/cpp/bvh_walk_replay.cpp ---------------------------------------------------------------------------------------------------
def write_replay_input(path, scene, o, d):
    """One file of float64: [n_triangles, n_rays, analytic extent, 0], then per triangle its three vertices and its flat index (10 values),
    then per ray origin, direction, the closest analytic hit's t (inf: none) and flat index (-1: none) (8 values)."""
    tris, flats, _ = flat_triangles(scene)
    t, f = analytic_hit(scene, o, d)
    head = np.array([len(tris), len(o), analytic_extent(scene), 0.0])
    body_t = np.concatenate([tris.reshape(-1, 9), flats[:, None].astype(np.float64)], 1)
    body_r = np.concatenate([o, d, t[:, None], f[:, None].astype(np.float64)], 1)
    np.concatenate([head, body_t.reshape(-1), body_r.reshape(-1)]).astype("<f8").tofile(path)


def read_replay_output(text):
    """the program's text -> (dict of the build's figures, int64 [n_rays, 3]: winning flat index (-1: none), most entries held, exact ties)"""
    lines = text.strip().splitlines()
    assert lines[0].startswith("build ") and lines[-1] == "ok", text[-2000:]
    words = lines[0].split()
    build = {words[i]: int(words[i + 1]) for i in range(1, len(words), 2)}
    return build, np.array([[int(w) for w in ln.split()] for ln in lines[1:-1]], dtype=np.int64).reshape(-1, 3)
