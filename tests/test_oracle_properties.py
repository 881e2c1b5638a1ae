"""Size-independent properties of the path, checked on the oracle: they are the
same properties the gpu tests check on the device at full size."""
import dataclasses

import numpy as np


def test_linearity_in_emission(pkg, oracle):
    scene = pkg.cornell_box()
    cam = pkg.cornell_camera(48, 48)
    rp = pkg.RenderParams(spp=6, min_bounces=1, absorb=0.4, seed=3)
    r = oracle.render(scene, cam, rp, backward=True)
    total = r["image"].sum((0, 1)) * rp.spp
    np.testing.assert_allclose(r["grads"][3] * np.array(scene.params[3]), total, rtol=1e-12)


def test_central_differences_match_reverse_mode(pkg, oracle):
    """Sampling never depends on albedo/emission values, so with the keyed RNG a central
    difference of the render is exact up to rounding and the cubic term."""
    cam = pkg.cornell_camera(32, 32)
    rp = pkg.RenderParams(spp=4, min_bounces=4, absorb=1.0, seed=2)
    base = pkg.cornell_box()
    g = oracle.render(base, cam, rp, backward=True)["grads"]
    h = 1e-4
    for p, c in [(0, 0), (1, 1), (2, 2), (3, 0)]:
        vals = []
        for sgn in (1, -1):
            s = pkg.cornell_box()
            q = list(s.params[p]); q[c] += sgn * h; s.params[p] = tuple(q)
            vals.append(oracle.render(s, cam, rp)["image"].sum((0, 1))[c] * rp.spp)
        fd = (vals[0] - vals[1]) / (2 * h)
        assert abs(fd - g[p, c]) <= 1e-6 * abs(g[p, c])


def test_adjoint_image_is_linear(pkg, oracle):
    scene = pkg.cornell_box()
    cam = pkg.cornell_camera(24, 16)
    rp = pkg.RenderParams(spp=4, min_bounces=2, absorb=0.3, seed=5)
    rs = np.random.RandomState(0)
    a1 = rs.uniform(0, 1, (16, 24, 3)).astype(np.float32)
    a2 = rs.uniform(0, 1, (16, 24, 3)).astype(np.float32)
    g1 = oracle.render(scene, cam, rp, backward=True, adjoint=a1)["grads"]
    g2 = oracle.render(scene, cam, rp, backward=True, adjoint=a2)["grads"]
    g12 = oracle.render(scene, cam, rp, backward=True, adjoint=(a1 + a2))["grads"]
    np.testing.assert_allclose(g1 + g2, g12, rtol=1e-6)
    ones = oracle.render(scene, cam, rp, backward=True, adjoint=np.ones((16, 24, 3), np.float32))["grads"]
    np.testing.assert_array_equal(ones, oracle.render(scene, cam, rp, backward=True)["grads"])


def test_shards_tile_the_frame(pkg, oracle):
    scene = pkg.cornell_box()
    cam = pkg.cornell_camera(40, 37)
    rp = pkg.RenderParams(spp=3, min_bounces=2, absorb=0.5, seed=8, band_rows=4)
    full = oracle.render(scene, cam, rp, backward=True)
    img = np.zeros_like(full["image"]); g = np.zeros_like(full["grads"]); seg = 0
    for s in range(3):
        r = oracle.render(scene, cam, dataclasses.replace(rp, shard=s, n_shards=3), backward=True)
        rows = pkg.shard_rows(37, 4, 3, s)
        img[rows] = r["image"][rows]; g += r["grads"]; seg += r["stats"]["segments"]
    np.testing.assert_array_equal(img, full["image"])
    np.testing.assert_allclose(g, full["grads"], rtol=1e-12)
    assert seg == full["stats"]["segments"]


def test_rng_is_uniform_and_decorrelated(oracle):
    """drt_rng_u31 replaces libc rand(): 31-bit, uniform, no visible correlation between
    neighbouring paths or consecutive draws."""
    n = 20000
    u = np.array([[oracle.rng_u31(1, p, d) for d in range(4)] for p in range(n)], dtype=np.float64) / 2147483647.0
    assert u.min() >= 0 and u.max() <= 1
    assert abs(u.mean() - 0.5) < 0.005 and abs(u.var() - 1 / 12) < 0.002
    for d in range(4):
        hist = np.histogram(u[:, d], bins=16, range=(0, 1))[0]
        chi2 = ((hist - n / 16) ** 2 / (n / 16)).sum()
        assert chi2 < 45            # 15 dof, p ~ 1e-4
    assert abs(np.corrcoef(u[:-1, 0], u[1:, 0])[0, 1]) < 0.03      # path p vs p+1
    assert abs(np.corrcoef(u[:, 0], u[:, 1])[0, 1]) < 0.03          # draw n vs n+1
    assert abs(np.corrcoef(u[:, 1], u[:, 2])[0, 1]) < 0.03
    # different seeds give different streams; 64-bit path ids are honoured
    assert oracle.rng_u31(1, 5, 0) != oracle.rng_u31(2, 5, 0)
    assert oracle.rng_u31(1, 5, 0) != oracle.rng_u31(1, 5 + (1 << 32), 0)


def _mix32(x):
    x = x.astype(np.uint32, copy=True)
    x ^= x >> np.uint32(16); x *= np.uint32(0x7feb352d)
    x ^= x >> np.uint32(15); x *= np.uint32(0x846ca68b)
    x ^= x >> np.uint32(16)
    return x


def _u31(seed, paths, n):
    """include/drt_hip.h's drt_rng_u31, vectorised over 64-bit path indices."""
    c = np.uint32(0x9E3779B9)
    paths = np.asarray(paths, dtype=np.uint64)
    with np.errstate(over="ignore"):
        stream = _mix32(np.uint32(seed) + c * ((paths >> np.uint64(32)).astype(np.uint32) + np.uint32(1)))
        h = _mix32(stream + c * np.uint32(n + 1))
        return _mix32(h ^ paths.astype(np.uint32)) >> np.uint32(1)


def test_no_two_paths_of_config_3_share_draws(oracle):
    """Independent streams: among ALL 16,777,216 camera samples of config 3 (512 x 512 x 64, seed 1)
    no pair of consecutive draws (n, n + 1), n = 0..5, occurs twice -- neither in two paths at the same position (a key
    collision) nor at different positions (one path replaying another's sequence shifted).  The 32-bit-key scheme of
    rounds 1-2 (draw = mix32(key32 + C (n + 1))) fails this scan with ~6e4 repeated pairs on a QUARTER of the paths."""
    rs = np.random.RandomState(0)
    for seed, path, n in zip(rs.randint(0, 2**31, 64), rs.randint(0, 2**40, 64, dtype=np.int64), rs.randint(0, 300, 64)):
        assert int(_u31(int(seed), np.array([path], np.uint64), int(n))[0]) == oracle.rng_u31(int(seed), int(path), int(n))
    for path in (2**31 - 1, 2**31, 2**32 - 1, 2**32):      # the sign bit of the 32-bit key, its last value and the first index past it
        for seed, n in ((1, 0), (2**31 + 5, 7), (2**32 - 1, 299)):
            assert int(_u31(seed, np.array([path], np.uint64), n)[0]) == oracle.rng_u31(seed, path, n)
    paths = np.arange(512 * 512 * 64, dtype=np.uint64)
    draws = [_u31(1, paths, n).astype(np.uint64) for n in range(7)]
    for d in draws[:2]:                       # at one draw index the paths get pairwise different 32-bit words (a bijection):
        assert np.unique(d, return_counts=True)[1].max() <= 2      # a 31-bit draw is shared by at most two of them
    windows = np.concatenate([(draws[i] << np.uint64(31)) | draws[i + 1] for i in range(6)])
    windows.sort()
    assert int((windows[1:] == windows[:-1]).sum()) == 0
    # the scan does find the defect it is looking for: the old scheme, a quarter of the paths
    c = np.uint32(0x9E3779B9)
    with np.errstate(over="ignore"):
        q = paths[: 1 << 22].astype(np.uint32)
        key = _mix32(_mix32(np.uint32(1) + c) ^ q)
        old = [(_mix32(key + c * np.uint32(n + 1)) >> np.uint32(1)).astype(np.uint64) for n in range(7)]
    w_old = np.concatenate([(old[i] << np.uint64(31)) | old[i + 1] for i in range(6)])
    w_old.sort()
    assert int((w_old[1:] == w_old[:-1]).sum()) > 10000


def test_keyed_and_libc_streams_agree_statistically(pkg, oracle):
    """Two sample sets of the same estimator: means agree within Monte-Carlo noise."""
    scene = pkg.cornell_box()
    cam = pkg.cornell_camera(64, 64)
    rp = pkg.RenderParams(spp=8, min_bounces=4, absorb=1.0, seed=1)
    a = oracle.render(scene, cam, rp)["image"].mean((0, 1))
    b = oracle.render(scene, cam, rp, rng_mode=oracle.RNG_LIBC, faithful=True)["image"].mean((0, 1))
    np.testing.assert_allclose(a, b, rtol=0.05)


def test_max_depth_cap_equals_absorb_one(pkg, oracle):
    """The depth cap (ABI extension) truncates exactly like `-b D -p 1` when roulette is off."""
    scene = pkg.cornell_box()
    cam = pkg.cornell_camera(20, 20)
    a = oracle.render(scene, cam, pkg.RenderParams(spp=4, min_bounces=5, absorb=1.0, seed=4), backward=True)
    b = oracle.render(scene, cam, pkg.RenderParams(spp=4, min_bounces=99, absorb=0.5, max_depth=5, seed=4), backward=True)
    np.testing.assert_array_equal(a["image"], b["image"])
    np.testing.assert_array_equal(a["grads"], b["grads"])


def test_a_cap_where_the_roulette_ends_every_path_anyway_is_transparent(pkg, oracle):
    """A user max_depth at or beyond min_bounces with absorb == 1 cuts nothing: the roulette of that depth ends the path with
    certainty and consumes its draw, as in the reference, which has no cap -- under the unbiased operator, where every later
    suffix of a chain depends on how many numbers were drawn before, the capped render is the uncapped one (round 4's route
    fuzz found the restatement skipping that draw; the device never did)."""
    scene = pkg.scene_by_name("cornell_mirror_wall")
    cam = pkg.cornell_camera(24, 18)
    free = oracle.render(scene, cam, pkg.RenderParams(spp=3, min_bounces=3, absorb=1.0, seed=294368374), backward=True, unbiased=True,
                         zero_dir_miss=True)
    for cap in (3, 4, 9):
        capped = oracle.render(scene, cam, pkg.RenderParams(spp=3, min_bounces=3, absorb=1.0, seed=294368374, max_depth=cap),
                               backward=True, unbiased=True, zero_dir_miss=True)
        assert capped["stats"]["segments"] == free["stats"]["segments"]
        np.testing.assert_array_equal(capped["grads"], free["grads"])
    cut = oracle.render(scene, cam, pkg.RenderParams(spp=3, min_bounces=3, absorb=1.0, seed=294368374, max_depth=2), backward=True,
                        unbiased=True, zero_dir_miss=True)
    assert cut["stats"]["segments"] < free["stats"]["segments"] and cut["stats"]["deepest"] == 2 and free["stats"]["deepest"] == 3


def test_a_roulette_draw_of_exactly_one_survives_absorb_one_and_divides_by_zero(pkg, oracle):
    """random::uniform() is rand() / RAND_MAX: 1.0 when rand() returns RAND_MAX, once in 2^31 draws.  With absorb == 1 such a
    path passes `uniform() < absorb` at min_bounces, goes on with survival probability p = 1 - absorb = 0 and its radiance is
    divided by it (pathtracer.hpp:128-133): inf or NaN in the reference -- and in the restatement, which follows it.  The
    device ends every path at min_bounces when absorb == 1 (finite; tests/test_gpu_parity.py).  Found by round 4's route fuzz:
    path 2133 of this render draws RAND_MAX at its depth-5 roulette (one frame in 128 of BASELINE config 3 has such a path)."""
    scene = pkg.scene_by_name("cornell_mirror_wall")
    cam = pkg.cornell_camera(15, 36)
    rp = pkg.RenderParams(spp=10, min_bounces=5, absorb=1.0, seed=83368279)
    assert oracle.rng_u31(rp.seed, 2133, 12) == 2147483647
    o = oracle.render(scene, cam, rp, backward=True)
    assert o["stats"]["deepest"] == 6 and not np.isfinite(o["grads"]).all() and not np.isfinite(o["image"][14, 3]).any()
    assert np.isfinite(np.delete(o["image"].reshape(-1, 3), 14 * 15 + 3, axis=0)).all()
