"""The inputs of tests/test_gpu_mesh_geometry.py, checked on the CPU -- so that the GPU tests cannot pass vacuously.

tests/cpp/bvh_walk_replay.cpp replays the device's ordered BVH walk in f64 on the tree drt_bvh.h builds (and checks itself against a
linear scan).  It is fed the pixel centres of each GPU case's frame and 2000 seeded wall-to-mesh rays, and says per ray how many stack
entries it held and how many exact ties it met.  The conditions below are thresholds on that: a family that misses one gets another size
or seed in tests/mesh_families.py, never another threshold.  The restatement (oracle/drt_oracle.c: a linear scan, no BVH) is run on every
GPU case too: finite, the parameters the case is about reached, the open sheet seen from behind."""
import os
import re
import subprocess

import numpy as np
import pytest

import mesh_families as mf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "differentiable-renderer_amd", "csrc")
N_SECONDARY, SECONDARY_SEED = 2000, 5
MIN_PRIMARY_OVERFLOW, MIN_SECONDARY_OVERFLOW = 15, 500
MIN_BACK_FACE_SHARE = 0.05


def defined(header, name):
    """the value the header gives the macro"""
    m = re.search(r"^#define\s+" + name + r"\s+(\d+)", open(os.path.join(CSRC, header)).read(), re.M)
    assert m, (header, name)
    return int(m.group(1))


@pytest.fixture(scope="module")
def replay_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("replay") / "bvh_walk_replay")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", os.path.join(ROOT, "tests", "cpp", "bvh_walk_replay.cpp"), "-o", exe],
                   check=True)
    return exe


_replayed = {}


@pytest.fixture
def replay(pkg, replay_exe, tmp_path):
    def run(name):
        """family `name`: (build figures, rows of the frame's primary rays, rows of the secondary rays); exit status 0 = the walk and the
        linear scan name the same winner for every ray"""
        if name not in _replayed:
            scene = mf.family(pkg, name)
            o1, d1 = mf.primary_rays(mf.camera(pkg))
            o2, d2 = mf.wall_rays(scene, N_SECONDARY, SECONDARY_SEED)
            path = str(tmp_path / (name + ".f64"))
            mf.write_replay_input(path, scene, np.concatenate([o1, o2]), np.concatenate([d1, d2]))
            r = subprocess.run([replay_exe, path], capture_output=True, text=True)
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
            build, rows = mf.read_replay_output(r.stdout)
            _replayed[name] = (build, rows[: len(o1)], rows[len(o1):])
            hit = rows[:, 0] >= 0
            print(f"{name}: {build}; primary rays: {int((rows[:len(o1), 0] >= 0).sum())} hit, most entries {rows[:len(o1), 1].max()}; "
                  f"secondary: {int((rows[len(o1):, 0] >= 0).sum())} hit, most entries {rows[len(o1):, 1].max()}; "
                  f"rays that hit and met a tie {int((hit & (rows[:, 2] > 0)).sum())} of {int(hit.sum())}")
        return _replayed[name]
    return run


REPLAYED = [n for n in mf.FAMILIES if n != "slivers_faces"]      # (the geometry of `slivers`)


@pytest.mark.parametrize("name", REPLAYED)
def test_no_ray_holds_more_than_the_stack_and_the_walk_finds_the_scan_s_winner(replay, name):
    build, primary, secondary = replay(name)
    assert build["stack_bound"] == defined("drt_device.h", "DRT_BVH_STACK") == defined("drt_bvh.h", "DRT_BVH_STACK")
    assert build["stack_need"] <= build["stack_bound"]
    assert max(primary[:, 1].max(), secondary[:, 1].max()) <= build["stack_need"]
    assert (primary[:, 0] >= 0).sum() > 0 and (secondary[:, 0] >= 0).sum() > 0        # the rays do meet the mesh


@pytest.mark.parametrize("name", mf.OVERFLOW)
def test_overflow_families_hold_more_than_the_lds_stack(replay, name):
    lds = defined("drt_path_mesh.h", "DRT_MESH_LDS_STACK")
    build, primary, secondary = replay(name)
    n1, n2 = int((primary[:, 1] > lds).sum()), int((secondary[:, 1] > lds).sum())
    print(f"{name}: rays that hold more than {lds} entries: {n1} primary, {n2} of {len(secondary)} secondary")
    assert n1 >= MIN_PRIMARY_OVERFLOW and n2 >= MIN_SECONDARY_OVERFLOW


def test_the_default_mesh_stays_inside_the_lds_stack(replay):
    """the control: the day the mesh of every earlier test starts to cover the overflow path, someone notices"""
    lds = defined("drt_path_mesh.h", "DRT_MESH_LDS_STACK")
    _, primary, secondary = replay("control")
    assert max(primary[:, 1].max(), secondary[:, 1].max()) <= lds


@pytest.mark.parametrize("name", mf.TIES)
def test_every_hit_on_coincident_faces_is_a_tie(replay, name):
    _, primary, secondary = replay(name)
    rows = np.concatenate([primary, secondary])
    hit = rows[:, 0] >= 0
    assert hit.sum() > 40 and (rows[hit, 2] > 0).all()
    # and the winner is the first of the coincident faces in scene order: one of the first quad's two triangles
    flat0 = 0                                    # (shape 0 is the mesh in these families)
    assert set(rows[hit, 0]) <= {flat0, flat0 + 1}


def test_nested_meets_the_stack_bound(replay):
    build, _, _ = replay("nested")
    print(f"nested: stack_need {build['stack_need']}, before any rebuild {build['first_stack_need']}, bound {build['stack_bound']}")
    assert build["stack_need"] == build["stack_bound"] or build["first_stack_need"] > build["stack_bound"]


# ---- the restatement alone, on every GPU case ------------------------------------------------------------------------------------------
def oracle_cases():
    """(family, tracer, unbiased operator): every render of tests/test_gpu_mesh_geometry.py's in-process tests"""
    for name in mf.BASE + ("slivers_faces",):
        for tracer in range(len(mf.TRACERS)):
            yield name, tracer, False
    for name in mf.UNBIASED:
        yield name, mf.UNBIASED_TRACER, True


@pytest.mark.parametrize("name,tracer,unbiased", list(oracle_cases()))
def test_the_restatement_takes_every_case(pkg, oracle, name, tracer, unbiased):
    scene = mf.family(pkg, name)
    cam = mf.camera(pkg, mf.FACES_FRAME if name == "slivers_faces" else mf.FRAME)
    rp = mf.render_params(pkg, tracer, spp=1, seed=mf.UNBIASED_SEED) if unbiased else mf.render_params(pkg, tracer, spp=mf.FACES_SPP if name == "slivers_faces" else mf.SPP)
    ref = oracle.render(scene, cam, rp, backward=True, unbiased=unbiased, zero_dir_miss=unbiased)
    assert np.isfinite(ref["image"]).all() and np.isfinite(ref["grads"]).all()
    reached, untouched = mf.ABOUT.get(name, ((), ()))
    for p in reached:
        g = ref["grads"][scene.param_names.index(p)]
        print(f"{name} tracer {tracer}{' unbiased' if unbiased else ''}: d/d{p} = {g}")
        assert np.abs(g).max() > 0, p
    for p in untouched:          # a later coincident face never wins: its colour gets exactly nothing
        assert not ref["grads"][scene.param_names.index(p)].any(), p


@pytest.mark.parametrize("name", ["open_sheet", "glowing_sheet"])
@pytest.mark.parametrize("tracer", range(len(mf.TRACERS)))
def test_the_open_sheet_is_seen_from_behind(pkg, oracle, name, tracer):
    """at least 5 % of the mesh hits of the frame's paths are back-face hits (dot(d, n) > 0), by the restatement's linear scan"""
    scene = mf.family(pkg, name)
    cam = mf.camera(pkg)
    rp = mf.render_params(pkg, tracer)
    n_paths = cam.width * cam.height * rp.spp
    v = oracle.render(scene, cam, rp, dump_paths=n_paths)["vertices"]
    _, flats, _ = mf.flat_triangles(scene)
    on_mesh = np.isin(v[:, 8].astype(np.int64), flats)
    back = (v[on_mesh, 5:8] * v[on_mesh, 13:16]).sum(1) > 0
    print(f"{name} tracer {tracer}: {int(on_mesh.sum())} mesh hits, {int(back.sum())} from behind ({back.mean():.1%})")
    assert on_mesh.sum() > 100 and back.mean() >= MIN_BACK_FACE_SHARE
