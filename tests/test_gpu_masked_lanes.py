"""k_path_lean's bounce beside a compiled-in program runs three per-lane special cases under the lane mask instead of computing them for all
64 lanes and keeping them by select (csrc/drt_path.h: DRT_LEAN_MASK_NORMAL, DRT_LEAN_REC_OFFSET, DRT_LEAN_MASK_REST; csrc/drt_prog.h:
closest_hit_sig's SCALE):
1. the sphere's normal only in the lanes that hit a sphere, behind a branch that a wave of plane hits skips;
2. the closest hit hands back the byte offset of the hit's record, the miss record's included;
3. the colour's row, the throughput and the counters move on only in the lanes whose path goes on.
Nothing of that may move a bit.

The oracle is the pair of tracers of tests/test_gpu_path_lean.py: A (absorb 1, min_bounces = d) takes k_path_lean; B (absorb 0.5,
min_bounces = d, max_depth = d) has a user cap and takes the unchanged k_path.  Same draws, same paths: image, gradients and segment count
agree BYTE FOR BYTE.  Both are also held against the fp64 restatement at the bounds of tests/test_gpu_parity.py (check_f32).

Everything is rendered once, by a child process (tests/masked_lanes_child.py).  Frames 64 x 48 and 70 x 3 at 8 spp -- the second ends in a
part-empty wave whose spare lanes have no pixel --; depth caps 1, 2, 3 and 8, so that lanes stop at every vertex; forward only, with
gradients, and with gradients from an adjoint image.  Scenes:
  cornell   the reference's scene: waves of sphere and plane hits mixed (the library's kernels)
  inside    the same from an eye inside the front sphere: every lane takes the normal's block at vertex 0
  box       the room without spheres, its ceiling the light: no lane ever hits a sphere, whole waves skip the block at every vertex; six
            shapes, so the kernels are hiprtc's and the miss record stands at another offset than the library's
  open      the same without near wall and ground: rays leave at every depth and read the miss record"""
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import masked_lanes_child as mlc
from test_gpu_parity import check_f32

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_restated = {}


@pytest.fixture(scope="module")
def device():
    d = tempfile.mkdtemp(prefix="drt_masked_lanes_")
    try:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "masked_lanes_child.py"), d], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, f"child: status {p.returncode}\n" + p.stdout[-3000:] + p.stderr[-3000:]
        with np.load(os.path.join(d, "outputs.npz")) as z:
            return {k: z[k] for k in z.files}
    finally:
        shutil.rmtree(d, ignore_errors=True)


def restated(pkg, oracle, name, frame, depth, mode):
    """the fp64 restatement of one case, computed once (the tracers trace the same paths with the same weights: A's numbers serve both; the
    forward-only render's image is the one of the render with gradients)"""
    k = (name, frame, depth, mode == "adj")
    if k not in _restated:
        make, camera, _, _ = mlc.SCENES[name]
        _restated[k] = oracle.render(make(pkg), camera(pkg, frame), mlc.tracers(pkg, depth)["A"], backward=True,
                                     adjoint=mlc.adjoint(frame) if mode == "adj" else None)
    return _restated[k]


@pytest.mark.parametrize("mode", mlc.MODES)
@pytest.mark.parametrize("depth", mlc.DEPTHS)
@pytest.mark.parametrize("name", list(mlc.SCENES))
def test_masked_lanes_keep_every_bit(pkg, oracle, device, name, depth, mode):
    backward = mode != "fwd"
    for frame in mlc.FRAMES:
        what = (name, frame, depth, mode)
        a, b = ({f: device[mlc.key(name, frame, depth, mode, t) + "/" + f] for f in ("image", "stats", "program") + (("grads",) if backward else ())}
                for t in "AB")
        print(*what, "segments", a["stats"][0], "capped", b["stats"][1], "mean", float(a["image"].mean()))
        assert str(a["program"]) == mlc.SCENES[name][3] and str(b["program"]) == mlc.SCENES[name][3], (what, a["program"], b["program"])
        assert a["stats"][2] == 1 and b["stats"][2] == 1, what                               # one launch of a path kernel each
        assert a["stats"][1] == 0, what                                                      # A: no user cap
        assert a["stats"][0] == b["stats"][0] and a["stats"][0] > 0, (what, a["stats"][0], b["stats"][0])
        assert a["image"].tobytes() == b["image"].tobytes(), (what, float(np.abs(a["image"] - b["image"]).max()))
        if backward:
            assert a["grads"].tobytes() == b["grads"].tobytes(), (what, float(np.abs(a["grads"] - b["grads"]).max()))
        ref = restated(pkg, oracle, name, frame, depth, mode)
        ref_image, ref_grads = np.asarray(ref["image"], np.float64), np.asarray(ref["grads"], np.float64)
        for t in (a, b):
            if not ref_image.any():
                # no path of the frame ends on the light (one vertex deep, from inside the sphere): nothing to scale an error by -- all is exactly 0
                assert not t["image"].any() and not ref_grads.any() and (not backward or not t["grads"].any()), what
                assert t["stats"][0] == ref["stats"]["segments"], what
            else:
                check_f32(t["image"], t["grads"] if backward else None, t["stats"][0], ref_image, ref_grads if backward else None,
                          ref["stats"]["segments"], n_paths=frame[0] * frame[1] * mlc.SPP)


def test_the_cases_are_what_they_say(device):
    """one vertex deep the camera's ray is the only segment: from inside the sphere no path ends on the light, in the open room the rays that
    leave light nothing, and the closed room of planes is lit in all but a few pixels by eight vertices (the fp64 restatement: 3066 of 3072
    and 209 of 210)"""
    for frame in mlc.FRAMES:
        assert not device[mlc.key("inside", frame, 1, "fwd", "A") + "/image"].any()
        assert device[mlc.key("inside", frame, 8, "fwd", "A") + "/image"].any()
        assert (device[mlc.key("box", frame, 8, "fwd", "A") + "/image"].max(-1) > 0).mean() > 0.99
        dark = device[mlc.key("open", frame, 8, "fwd", "A") + "/image"].max(-1) == 0
        assert dark.any() and not dark.all(), frame
