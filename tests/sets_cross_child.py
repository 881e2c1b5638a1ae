"""The child process of tests/test_gpu_sets_cross.py::test_sample_ranges: DRT_HIP_PATH_SPR is read once per process, so the same frame
under another cut of its samples into ranges needs a process of its own.  cornell, 32 x 28, depth 5, spp 7, three sets, f32 and f64;
prints one JSON line: per mode the sample ranges the path launch ran, loss, bias, their sums of absolute terms, images, variance."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry  # noqa: E402

pkg = entry.load_package()
from test_gpu_sets_cross import TRACER, scales, sets_cross, target_for, three_sets  # noqa: E402


def n_ranges(stats, n_pixels, rows):
    """the sample ranges the path launch ran, from its statistics: path_bytes counts, per range, 8 bytes for each of a pixel's `rows`
    sums (no plain image in this call: no radiance partials), and two 4-byte counters per wave of 64 pixels"""
    per_range = n_pixels * rows * 8 + 8 * ((n_pixels + 63) // 64)
    assert stats["path_bytes"] % per_range == 0, (stats["path_bytes"], per_range)
    return stats["path_bytes"] // per_range


scene = pkg.scene_by_name("cornell")
cam = pkg.cornell_camera(32, 28)
hip = pkg.HipRenderer(0)
hip.upload_scene(scene)
P = three_sets(scene, 11)
target = target_for(cam)
out = {}
for mode, f64 in (("f32", False), ("f64", True)):
    res = sets_cross(hip, cam, pkg.RenderParams(spp=7, seed=9, **TRACER), P, target, f64)
    sc = scales(res, target, 7)
    out[mode] = {"ranges": n_ranges(res["stats"], 32 * 28, 18), "scale_loss": sc["loss"].tolist(), "scale_bias": sc["bias"].tolist(),
                 **{k: res[k].tolist() for k in ("loss", "bias", "images", "variance")}}
print(json.dumps(out))
hip.close()
